// Arithmetic self-check: the bitwise contract assumes gfx950 fp32 ops round
// exactly like IEEE-754 / the host (tests/test_gpu_parity.py::test_fp32_ops).
// Below it, the stateless device primitives called on their own
// (tests/test_gpu_primitives.py): the key sort and the batched fill.
#include <algorithm>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "step.h"
#include "../../include/tropical_hip_debug.h"

namespace {
__global__ void k_ops(const float* a, const float* b, const float* c, int64_t n, float* o) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  o[8 * i + 0] = sqrtf(a[i]);
  o[8 * i + 1] = __fdiv_rn(a[i], b[i]);
  o[8 * i + 2] = __fmaf_rn(a[i], b[i], c[i]);
  o[8 * i + 3] = __fmul_rn(a[i], b[i]);
  o[8 * i + 4] = __fadd_rn(a[i], b[i]);
  o[8 * i + 5] = sqrtf(a[i]);
  o[8 * i + 6] = a[i] / b[i];
  o[8 * i + 7] = tanhf(a[i]);
}
}  // namespace

extern "C" int tnp_debug_ops(const float* a, const float* b, const float* c, int64_t n, float* out,
                             void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_ops, dim3(tnp_grid(n)), dim3(TNP_BLOCK), 0, (hipStream_t)stream, a, b, c, n, out);
  TNP_CHECK(hipGetLastError());
  return 0;
}

// the connecting-edge key sort on its own (sort.hip sort_keys_lex), called as
// finish_connect calls it: private a / b buffers and a scratch of exactly
// sort_lex_scratch_bytes; the caller's keys are only read
extern "C" int tnp_debug_sort_keys_lex(const uint64_t* d_keys, int64_t n, int nb, int R, uint64_t* d_out,
                                       void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || nb < 1 || nb > 32 || (n > 0 && (!d_keys || !d_out))) {
    tnp_set_error("tnp_debug_sort_keys_lex: bad argument");
    return -1;
  }
  const size_t kb = (size_t)std::max<int64_t>(n, 1) * sizeof(uint64_t);
  const size_t need = sort_lex_scratch_bytes(n, nb, R);
  uint64_t *a = nullptr, *b = nullptr, *out = nullptr;
  void* scr = nullptr;
  int rc = 0;
  if (hipMalloc(&a, kb) != hipSuccess || hipMalloc(&b, kb) != hipSuccess ||
      hipMalloc(&scr, std::max<size_t>(need, 16)) != hipSuccess) {
    tnp_set_error("tnp_debug_sort_keys_lex: hipMalloc failed");
    rc = -1;
  }
  if (rc == 0 && n > 0 &&
      hipMemcpyAsync(a, d_keys, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    tnp_set_error("tnp_debug_sort_keys_lex: copy in failed");
    rc = -1;
  }
  if (rc == 0) rc = sort_keys_lex(a, b, n, nb, R, scr, need, &out, s);
  if (rc == 0 && n > 0 &&
      hipMemcpyAsync(d_out, out, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    tnp_set_error("tnp_debug_sort_keys_lex: copy out failed");
    rc = -1;
  }
  if (hipStreamSynchronize(s) != hipSuccess && rc == 0) {
    tnp_set_error("tnp_debug_sort_keys_lex: stream synchronise failed");
    rc = -1;
  }
  (void)hipFree(a);
  (void)hipFree(b);
  (void)hipFree(scr);
  return rc;
}

// the batched fill on its own (scan.hip launch_fill): k ranges, one call
extern "C" int tnp_debug_fill(void* const* h_ptrs, const uint64_t* h_sizes, const uint32_t* h_bytes, int k,
                              void* stream) {
  if (k < 0 || (k > 0 && (!h_ptrs || !h_sizes || !h_bytes))) {
    tnp_set_error("tnp_debug_fill: bad argument");
    return -1;
  }
  std::vector<FillOp> ops((size_t)k);
  for (int i = 0; i < k; ++i) ops[i] = FillOp{h_ptrs[i], h_sizes[i], h_bytes[i]};
  return launch_fill(ops.data(), k, (hipStream_t)stream);
}
