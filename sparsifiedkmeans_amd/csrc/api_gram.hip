// libspkm.so, host side of the Gram sums (spkm.h: spkm_gram_csc_dev, spkm_gram_csc_nnz_dev, spkm_last_gram_plan).  A
// translation unit of its own: the kernels of gram.hip and the call that plans (policy.h, spkm_gram_plan) and launches them.
#include "gram.hip"

#include "api_internal.h"

static int gram_check(spkm_ctx* ctx, uint64_t p2, uint64_t ncols, const int64_t* d_jc, const void* d_ir, int ir_bits,
                      const double* d_x, double* d_G)
{
    if (!ctx) return SPKM_ERR_NULL_ARG;
    if (p2 == 0) return SPKM_ERR_BAD_VALUE;
    if (p2 > (uint64_t)spkm_gram_max_p2 || ir_bits != 16) return SPKM_ERR_UNSUPPORTED;
    if (ncols && (!d_jc || !d_ir || !d_x || !d_G || ncols > 0x7fffffffffffull)) return SPKM_ERR_BAD_VALUE;
    return SPKM_OK;
}

// the caller states the chunk's entry count (the byte model's one input that lives on the device): nothing is read back
extern "C" int spkm_gram_csc_nnz_dev(spkm_ctx* ctx, uint64_t p2, uint64_t ncols, uint64_t nnz, const int64_t* d_jc,
                                     const void* d_ir, int ir_bits, const double* d_x, double* d_G, double* d_sum)
{
    const int st = gram_check(ctx, p2, ncols, d_jc, d_ir, ir_bits, d_x, d_G);
    if (st != SPKM_OK || ncols == 0) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    const spkm_gram_geom g = spkm_gram_plan((long long)p2, (unsigned long long)nnz, ncols, ctx->lds_max, ctx->sw.x_gram_tile,
                                            ctx->sw.x_gram_form);
    if (g.grid <= 0 || g.grid > 0x7fffffffLL) return SPKM_ERR_UNSUPPORTED; // (cannot happen within the ranges above)
    if (g.form == 1) {
        const size_t lds = spkm_gram_lds(g.T);
        HIP_TRY(allow_lds(ctx, (const void*)k_gram_tiles, lds));
        const int nb = (int)((p2 + g.T - 1) / g.T);
        hipLaunchKernelGGL(k_gram_tiles, dim3((unsigned)g.grid), dim3(64 * spkm_gram_waves), lds, ctx->stream,
                           (const long long*)d_jc, (const unsigned short*)d_ir, d_x, (long long)ncols, (int)p2, g.T, nb,
                           g.pairs, g.chunk, d_G, d_sum);
    } else {
        hipLaunchKernelGGL(k_gram_direct, dim3((unsigned)g.grid), dim3(256), 0, ctx->stream, (const long long*)d_jc,
                           (const unsigned short*)d_ir, d_x, (long long)ncols, (int)p2, d_G, d_sum);
    }
    HIP_TRY(hipGetLastError());
    ctx->last_gram[0] = g.form; ctx->last_gram[1] = g.T; ctx->last_gram[2] = g.pairs; ctx->last_gram[3] = g.grid;
    return SPKM_OK;
}

// ... or does not: a forced form needs no entry count (its tile, pairs and grid do not depend on it) and the call stays
// asynchronous; otherwise d_jc[ncols] is read back, 8 bytes, and the call waits once for what the stream holds in front of
// it (as spkm_shard_export_dev does on a ragged range)
extern "C" int spkm_gram_csc_dev(spkm_ctx* ctx, uint64_t p2, uint64_t ncols, const int64_t* d_jc, const void* d_ir, int ir_bits,
                                 const double* d_x, double* d_G, double* d_sum)
{
    const int st = gram_check(ctx, p2, ncols, d_jc, d_ir, ir_bits, d_x, d_G);
    if (st != SPKM_OK || ncols == 0) return st;
    long long nnz = 0;
    if (ctx->sw.x_gram_form == 0) {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipMemcpyAsync(&nnz, d_jc + ncols, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (nnz < 0) return SPKM_ERR_BAD_VALUE;
    }
    return spkm_gram_csc_nnz_dev(ctx, p2, ncols, (uint64_t)nnz, d_jc, d_ir, ir_bits, d_x, d_G, d_sum);
}

extern "C" int spkm_last_gram_plan(spkm_ctx* ctx, int64_t info[4])
{
    if (!ctx || !info) return SPKM_ERR_NULL_ARG;
    for (int k = 0; k < 4; k++) info[k] = ctx->last_gram[k];
    return SPKM_OK;
}
