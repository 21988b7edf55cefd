// (part of api_lloyd.hip) A shard's columns out as CSC, a chunk's entries in as records: the two calls a save and a load
// of a resident shard stream through (spkm.h: spkm_shard_export_dev, spkm_pack_records_dev; kernels: shard_io.hip).

extern "C" int spkm_shard_layout_info(const spkm_shard* s, int64_t info[3])
{
    if (!s || !info) return SPKM_ERR_NULL_ARG;
    info[0] = s->x != nullptr ? 1 : 0;
    info[1] = s->rec != nullptr ? 1 : 0;
    info[2] = s->fixed_s;
    return SPKM_OK;
}

// Columns [col0, col0 + ncols) of a shard as CSC in the caller's point order, from whichever layout holds the entries:
//   * CSC arrays resident (fixed stride or ragged): jc rebased by one small kernel, ir / x by two device-to-device copies of
//     the range -- nothing to convert;
//   * records only (spkm_shard_create_rec_dev, or after spkm_shard_release_csc): k_unpack_records_range reads records
//     col0 .. and writes the chunk.  ensure_csc is NOT called: no array of the shard's size is allocated, the shard stays
//     records-only.
// Neither source is touched by regroup_shard: the library's own order lives in the screen copy, the bounds and the index
// map (spkm_shard.map) alone, the records and the CSC arrays keep the caller's order -- the export never reads the map,
// and a regrouped shard exports what it was built from (tests/test_gpu_shard_io.py drives one there).
extern "C" int spkm_shard_export_dev(spkm_ctx* ctx, const spkm_shard* s, uint64_t col0, uint64_t ncols, int64_t* d_jc,
                                     void* d_ir, int ir_bits, double* d_x, uint64_t cap)
{
    if (!ctx || !s || !d_jc) return SPKM_ERR_NULL_ARG;
    if (col0 > s->n || ncols > s->n - col0) return SPKM_ERR_BAD_VALUE;
    if (ir_bits != s->ir_bits) return SPKM_ERR_BAD_VALUE;
    HIP_TRY(hipSetDevice(ctx->device));
    const bool from_rec = s->x == nullptr && s->rec != nullptr && s->fixed_s > 0;
    const bool jc_only = d_ir == nullptr && d_x == nullptr; // (the range's column starts alone: nothing is read back)
    long long j0, j1;
    if (jc_only) j0 = j1 = 0;
    else if (s->fixed_s > 0) { j0 = (long long)col0 * s->fixed_s; j1 = j0 + (long long)ncols * s->fixed_s; }
    else if (s->nnz == 0) j0 = j1 = 0;
    else {
        // a ragged range's entry count is known to the device alone: one read-back (the call blocks, as
        // spkm_shard_get_column_host does)
        long long a = 0, b = 0;
        HIP_TRY(hipMemcpyAsync(&a, s->jc + col0, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(&b, s->jc + col0 + ncols, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        j0 = a; j1 = b;
    }
    const uint64_t cnt = (uint64_t)(j1 - j0);
    if (cnt && !from_rec && s->x == nullptr) return SPKM_ERR_BAD_VALUE; // (cannot happen: entries without a layout)
    // (d_jc first: it is all a call without d_ir and d_x asks for, and after a refusal for cap d_jc[ncols] tells the caller
    //  how much room the range needs)
    const unsigned gj = (unsigned)std::min<uint64_t>((ncols + 256) / 256, 4096);
    if (s->fixed_s > 0)
        hipLaunchKernelGGL(k_fill_jc, dim3(gj), dim3(256), 0, ctx->stream, (long long*)d_jc, (long long)ncols, (long long)s->fixed_s);
    else
        hipLaunchKernelGGL(k_export_jc, dim3(gj), dim3(256), 0, ctx->stream, (const long long*)s->jc, (long long)col0,
                           (long long)ncols, (long long*)d_jc);
    HIP_TRY(hipGetLastError());
    if (jc_only) return SPKM_OK;
    if (cap < cnt) return SPKM_ERR_BAD_VALUE;
    if (cnt == 0) return SPKM_OK;
    if (!d_ir || !d_x) return SPKM_ERR_NULL_ARG;
    const size_t irb = (size_t)s->ir_bits / 8;
    if (!from_rec) {
        HIP_TRY(hipMemcpyAsync(d_x, s->x + j0, cnt * 8, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_ir, (const char*)s->ir + (size_t)j0 * irb, cnt * irb, hipMemcpyDeviceToDevice, ctx->stream));
        return SPKM_OK;
    }
    const int R = s->rec_R;
    if ((uintptr_t)s->rec % 16 != 0) return SPKM_ERR_BAD_VALUE; // (records are 16-byte aligned: spkm.h)
    const int vec16 = ((uintptr_t)d_x % 16 == 0 && (uintptr_t)d_ir % 16 == 0) ? 1 : 0;
    const uint64_t groups = (ncols + SIO_PTS - 1) / SIO_PTS;
    const unsigned grid = (unsigned)std::min<uint64_t>(groups, (uint64_t)std::max(1, ctx->num_cus) * 8);
    const size_t lds = (size_t)SIO_PTS * R;
    if (s->ir_bits == 16)
        hipLaunchKernelGGL((k_unpack_records_range<unsigned short>), dim3(grid), dim3(256), lds, ctx->stream, (const char*)s->rec,
                           (long long)col0, (long long)ncols, s->fixed_s, R, vec16, (unsigned short*)d_ir, d_x);
    else
        hipLaunchKernelGGL((k_unpack_records_range<unsigned int>), dim3(grid), dim3(256), lds, ctx->stream, (const char*)s->rec,
                           (long long)col0, (long long)ncols, s->fixed_s, R, vec16, (unsigned int*)d_ir, d_x);
    HIP_TRY(hipGetLastError());
    return SPKM_OK;
}

// The inverse for a fixed-stride chunk: ncols columns of s <= 64 entries each (d_ir / d_x: ncols * s entries in column
// order) become ncols records at d_rec_out, k_build_records's layout with the padding bytes zeroed.
extern "C" int spkm_pack_records_dev(spkm_ctx* ctx, uint64_t p, uint64_t s, int ir_bits, uint64_t ncols, const void* d_ir,
                                     const double* d_x, void* d_rec_out)
{
    if (!ctx || (ncols && (!d_ir || !d_x || !d_rec_out))) return SPKM_ERR_NULL_ARG;
    if (ir_bits != 16 && ir_bits != 32) return SPKM_ERR_BAD_VALUE;
    if (p == 0 || (ir_bits == 16 && p > 65536) || s == 0 || s > 64 || s > p || ncols > 0x7ff00000ull) return SPKM_ERR_BAD_VALUE;
    if (ncols && (uintptr_t)d_rec_out % 16 != 0) return SPKM_ERR_BAD_VALUE; // (records are 16-byte aligned: spkm.h)
    HIP_TRY(hipSetDevice(ctx->device));
    if (ncols == 0) return SPKM_OK;
    const int R = (int)spkm_record_bytes(s, ir_bits);
    const int vec16 = ((uintptr_t)d_x % 16 == 0 && (uintptr_t)d_ir % 16 == 0) ? 1 : 0;
    const uint64_t groups = (ncols + SIO_PTS - 1) / SIO_PTS;
    const unsigned grid = (unsigned)std::min<uint64_t>(groups, (uint64_t)std::max(1, ctx->num_cus) * 8);
    const size_t lds = (size_t)SIO_PTS * R;
    if (ir_bits == 16)
        hipLaunchKernelGGL((k_build_records_range<unsigned short>), dim3(grid), dim3(256), lds, ctx->stream,
                           (const unsigned short*)d_ir, d_x, (long long)ncols, (int)s, R, vec16, (char*)d_rec_out);
    else
        hipLaunchKernelGGL((k_build_records_range<unsigned int>), dim3(grid), dim3(256), lds, ctx->stream,
                           (const unsigned int*)d_ir, d_x, (long long)ncols, (int)s, R, vec16, (char*)d_rec_out);
    HIP_TRY(hipGetLastError());
    return SPKM_OK;
}
