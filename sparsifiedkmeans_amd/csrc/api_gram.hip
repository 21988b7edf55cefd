// libspkm.so, host side of the Gram sums (spkm.h: spkm_gram_csc_dev, spkm_gram_csc_nnz_dev, spkm_last_gram_plan) and of the
// Gram operator on a thin block (spkm_cov_apply_csc_dev, spkm_last_cov_apply_plan).  A translation unit of its own: the
// kernels of gram.hip and gram_apply.hip and the calls that plan (policy.h, spkm_gram_plan / spkm_cov_apply_plan) and
// launch them.
#include "gram.hip"
#include "gram_apply.hip"

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

// ---- the Gram operator on a thin block (spkm.h: spkm_cov_apply_csc_dev; kernels: gram_apply.hip) ----
template <typename IR>
static int cov_apply_launch(spkm_ctx* ctx, const spkm_cov_apply_geom& g, uint64_t p2, uint64_t ncols, const int64_t* d_jc,
                            const void* d_ir, const double* d_x, int b, const double* d_Q, double* d_Z, double* d_work,
                            double* d_diag, double* d_sum)
{
    const long long* jc = (const long long*)d_jc;
    const IR* ir = (const IR*)d_ir;
    int lb = 0;
    while ((1 << lb) < b) lb++;
    if (g.form == 1) {
        const int bb = b + (d_diag != nullptr) + (d_sum != nullptr);
        int lbb = 0;
        while ((1 << lbb) < bb) lbb++;     // (bb <= 34: at most 64, one entry per step)
        const size_t lds = spkm_cov_apply_lds(g.R, bb);
        HIP_TRY(allow_lds(ctx, (const void*)k_cov_scatter_slab<IR>, lds));
        hipLaunchKernelGGL(k_cov_project<IR>, dim3((unsigned)g.pgrid), dim3(256), 0, ctx->stream, jc, ir, d_x, (long long)ncols,
                           (unsigned long long)p2, b, lb, d_Q, d_work);
        hipLaunchKernelGGL(k_cov_scatter_slab<IR>, dim3((unsigned)g.grid), dim3(64 * spkm_cov_waves), lds, ctx->stream, jc, ir,
                           d_x, (long long)ncols, (unsigned long long)p2, b, lbb, g.R, g.slices, g.chunk,
                           (const double*)d_work, d_Z, d_diag, d_sum);
    } else {
        hipLaunchKernelGGL(k_cov_apply_direct<IR>, dim3((unsigned)g.grid), dim3(256), 0, ctx->stream, jc, ir, d_x,
                           (long long)ncols, (unsigned long long)p2, b, lb, d_Q, d_Z, d_diag, d_sum);
    }
    HIP_TRY(hipGetLastError());
    return SPKM_OK;
}

extern "C" int spkm_cov_apply_csc_dev(spkm_ctx* ctx, uint64_t p2, uint64_t ncols, uint64_t nnz, const int64_t* d_jc,
                                      const void* d_ir, int ir_bits, const double* d_x, uint32_t b, const double* d_Q,
                                      double* d_Z, double* d_work, double* d_diag, double* d_sum)
{
    if (!ctx) return SPKM_ERR_NULL_ARG;
    if (p2 == 0 || b == 0 || b > (uint32_t)spkm_cov_max_b) return SPKM_ERR_BAD_VALUE;
    if (ir_bits != 16 && ir_bits != 32) return SPKM_ERR_BAD_VALUE;
    if (ir_bits == 16 && p2 > 65536) return SPKM_ERR_BAD_VALUE;
    if (ncols && (!d_jc || !d_ir || !d_x || !d_Q || !d_Z || ncols > 0x7fffffffffffull)) return SPKM_ERR_BAD_VALUE;
    if (ncols == 0) return SPKM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const int extra = (d_diag != nullptr) + (d_sum != nullptr);
    const spkm_cov_apply_geom g = spkm_cov_apply_plan(p2, nnz, ncols, (int)b, extra, ir_bits, d_work != nullptr, ctx->lds_max,
                                                      ctx->sw.x_covapply_rows, ctx->sw.x_covapply_form);
    if (g.grid <= 0 || g.grid > 0x7fffffffLL) return SPKM_ERR_UNSUPPORTED; // (more slices than a launch has workgroups)
    const int st = ir_bits == 16 ? cov_apply_launch<unsigned short>(ctx, g, p2, ncols, d_jc, d_ir, d_x, (int)b, d_Q, d_Z, d_work, d_diag, d_sum)
                                 : cov_apply_launch<unsigned int>(ctx, g, p2, ncols, d_jc, d_ir, d_x, (int)b, d_Q, d_Z, d_work, d_diag, d_sum);
    if (st != SPKM_OK) return st;
    ctx->last_cov_apply[0] = g.form; ctx->last_cov_apply[1] = g.R; ctx->last_cov_apply[2] = g.slices; ctx->last_cov_apply[3] = g.grid;
    return SPKM_OK;
}

extern "C" int spkm_last_cov_apply_plan(spkm_ctx* ctx, int64_t info[4])
{
    if (!ctx || !info) return SPKM_ERR_NULL_ARG;
    for (int k = 0; k < 4; k++) info[k] = ctx->last_cov_apply[k];
    return SPKM_OK;
}
