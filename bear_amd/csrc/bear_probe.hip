// bear_probe.hip -- the probe entry of include/bear_hip.h: one device math routine per launch, element by element (tests and
// diagnostics only; no production path calls it).  The only unit that includes -- and so emits -- math_probe_kernel.
#include "bear_host.h"
#include "kernels_probe.h"

extern "C" {

int bear_math_probe_f64(bear_ws *ws, int op, const double *a, const double *b, uint64_t n, double *out0, double *out1,
                        void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (op < 0 || op >= BEAR_PROBE_N_OPS) return BEAR_ERR_INVALID_ARG;
  if (n == 0) return BEAR_OK;
  if (!a || !out0 || (probe_is_item(op) && (!b || !out1))) return BEAR_ERR_INVALID_ARG;
  const uint64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffull) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), op, a,
                     probe_is_item(op) ? b : nullptr, n, reinterpret_cast<const double2 *>(ws->logtab), out0,
                     probe_is_item(op) ? out1 : nullptr);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

}  // extern "C"
