// tests/emu_prim/emu_prim_api.cpp — TEST INFRASTRUCTURE: the device-primitive test kernels on the host emulator, behind the SAME entry points as the device library
// (tests/devprim/devprim.hip is compiled here with DEVPRIM_EMU).  With EMU_EST_BITS defined, the two hardware estimates are not the emulator's exact stand-ins but the
// exact value times (1 ± 2^-EMU_EST_BITS): the correction steps of qm_frcp / qm_recip / qm_rsqrt / ... then run on an estimate as bad as the one the project claims.
// emu_prim_est_sign selects the sign: 0 alternates with the low mantissa bit of the argument, +1 / -1 are fixed.  Never linked into the product.
#include <cmath>
#include <cstdint>
#include <cstring>
#ifdef EMU_EST_BITS
static int g_est_sign = 0;
static inline double emu_est(double exact, double arg) {
  uint64_t b; memcpy(&b, &arg, 8); const double s = g_est_sign ? (double)g_est_sign : ((b & 1) ? -1.0 : 1.0);
  return exact * (1.0 + s * std::ldexp(1.0, -(EMU_EST_BITS)));
}
static inline double emu_est_rcp(double x) { return emu_est(1.0 / x, x); }
static inline double emu_est_rsq(double x) { return emu_est(1.0 / std::sqrt(x), x); }
#define __builtin_amdgcn_rcp(x) emu_est_rcp((double)(x))
#define __builtin_amdgcn_rsq(x) emu_est_rsq((double)(x))
#endif
#include "hip_emu.h"
#define DEVPRIM_EMU
#include "../devprim/devprim.hip"

extern "C" {
// bits of the modelled estimates (0: the exact stand-ins) and the sign mode of their error
int emu_prim_est_bits() {
#ifdef EMU_EST_BITS
  return EMU_EST_BITS;
#else
  return 0;
#endif
}
void emu_prim_est_sign(int s) {
#ifdef EMU_EST_BITS
  g_est_sign = s > 0 ? 1 : (s < 0 ? -1 : 0);
#endif
}
}
