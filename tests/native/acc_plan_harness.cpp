// Test harness (CPU, g++): a C face on the accumulation's policy in sparsifiedkmeans_amd/csrc/policy.h -- spkm_accumulate_form,
// spkm_acc_max_slices -- for tests/test_acc_plan.py.  Not part of the product.
#include "../../sparsifiedkmeans_amd/csrc/policy.h"

extern "C" {
// out[4] = { form, R, slices, threads per workgroup }; returns the form
int acc_form(long long p, unsigned long long lds_max, int sliced, int x_slab_rows, int* out)
{
    const spkm_acc_plan a = spkm_accumulate_form(p, (size_t)lds_max, sliced != 0, x_slab_rows);
    out[0] = a.form; out[1] = a.R; out[2] = a.slices; out[3] = a.wg;
    return a.form;
}
int acc_max_slices() { return spkm_acc_max_slices; }
int acc_row_bytes() { return spkm_acc_row_bytes; }
int acc_static_lds() { return 0; } // k_accumulate_sliced declares no static LDS: the slab is all of its allocation
}
