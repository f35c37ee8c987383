// AddressSanitizer run of the HOST side of libpacingpseudo_opt (include/pacingpseudo_opt.h): the argument checks of every
// popt_* entry point, built for the host only (`make asan-opt`, no GPU needed).  Every call below must be rejected BEFORE
// anything is launched: return code < 0, a message in popt_last_error(), no out-of-bounds access while the check builds its message.
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "pacingpseudo_opt.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                              \
  do {                                                                                   \
    const int rc = (call);                                                               \
    const char* msg = popt_last_error();                                                 \
    if (rc >= 0 || !msg || !msg[0]) { printf("NOT REJECTED: %s -> %d\n", #call, rc); ++failures; } \
  } while (0)

// host memory standing in for device buffers: nothing may be launched, so nothing dereferences them on a device
alignas(256) static float p[64], g[64], m[64], v[64], e[64], lrd[4], clipd[4];
alignas(256) static int stepd[4], skipd[4];
alignas(256) static unsigned char ex[64];

// the three entry points behind one signature; which = 0 plain, 1 clip, 2 ema without a clip pointer, 3 ema with one
static int call(int which, float* p_, const float* g_, float* m_, float* v_, long long n, float lr, const float* lr_dev, float b1, float b2,
                float eps, float wd, int* step_dev, int* skip, const unsigned char* exempt, float* ema = e, double decay = 0.9,
                const float* clip = clipd) {
  switch (which) {
    case 0: return popt_adamw_step(p_, g_, m_, v_, n, lr, lr_dev, b1, b2, eps, wd, step_dev, skip, 1, exempt, nullptr);
    case 1: return popt_adamw_step_clip(p_, g_, m_, v_, n, lr, lr_dev, b1, b2, eps, wd, step_dev, skip, 1, exempt, clip, nullptr);
    case 2: return popt_adamw_step_ema(p_, g_, m_, v_, n, lr, lr_dev, b1, b2, eps, wd, step_dev, skip, 1, exempt, ema, decay, nullptr, nullptr);
    default: return popt_adamw_step_ema(p_, g_, m_, v_, n, lr, lr_dev, b1, b2, eps, wd, step_dev, skip, 1, exempt, ema, decay, clip, nullptr);
  }
}

static float* off(float* a, int bytes) { return (float*)((char*)a + bytes); }

int main() {
  if (popt_version() < 100) ++failures;
  if (!popt_last_error()) ++failures;
  if (popt_trip_elements() < 4 * 256) { printf("popt_trip_elements: at least one block of lanes\n"); ++failures; }

  const float lr = 1e-3f, b1 = 0.9f, b2 = 0.999f, eps = 1e-8f, wd = 0.1f;
  for (int w = 0; w < 4; ++w) {
    // null pointers
    EXPECT_REJECT(call(w, nullptr, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, nullptr, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, nullptr, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, nullptr, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, nullptr, skipd, ex));
    // n
    EXPECT_REJECT(call(w, p, g, m, v, 0, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, -4, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    // alignment: the slabs to 16 bytes, the mask to 4, the device scalars to 4
    EXPECT_REJECT(call(w, off(p, 4), g, m, v, 32, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, off(g, 8), m, v, 32, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, off(m, 12), v, 32, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, off(v, 4), 32, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 32, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex + 1));
    EXPECT_REJECT(call(w, p, g, m, v, 32, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex + 2));
    EXPECT_REJECT(call(w, p, g, m, v, 32, lr, off(lrd, 2), b1, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 32, lr, lrd, b1, b2, eps, wd, (int*)((char*)stepd + 1), skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 32, lr, lrd, b1, b2, eps, wd, stepd, (int*)((char*)skipd + 2), ex));
    // hyper-parameters: negative or not finite
    EXPECT_REJECT(call(w, p, g, m, v, 64, -1e-3f, nullptr, b1, b2, eps, wd, stepd, nullptr, nullptr));
    EXPECT_REJECT(call(w, p, g, m, v, 64, NAN, nullptr, b1, b2, eps, wd, stepd, nullptr, nullptr));
    EXPECT_REJECT(call(w, p, g, m, v, 64, INFINITY, nullptr, b1, b2, eps, wd, stepd, nullptr, nullptr));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, -1e-8f, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, NAN, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, INFINITY, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, -0.1f, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, NAN, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, INFINITY, stepd, skipd, ex));
    // betas outside [0, 1)
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, 1.f, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, -0.1f, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, NAN, b2, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, 1.f, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, -0.5f, eps, wd, stepd, skipd, ex));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, NAN, eps, wd, stepd, skipd, ex));
  }
  // the clip form needs its coefficient, aligned
  EXPECT_REJECT(call(1, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, e, 0.9, nullptr));
  EXPECT_REJECT(call(1, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, e, 0.9, off(clipd, 2)));
  EXPECT_REJECT(call(3, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, e, 0.9, off(clipd, 1)));
  // the ema form needs its shadow slab, 16-byte aligned, and a decay in (0, 1)
  for (int w = 2; w < 4; ++w) {
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, nullptr, 0.9));
    EXPECT_REJECT(call(w, p, g, m, v, 32, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, off(e, 4), 0.9));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, e, 0.0));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, e, 1.0));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, e, -0.5));
    EXPECT_REJECT(call(w, p, g, m, v, 64, lr, lrd, b1, b2, eps, wd, stepd, skipd, ex, e, (double)NAN));
  }

  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("asan_opt_args: all argument checks rejected their input, no sanitizer report\n");
  return 0;
}
