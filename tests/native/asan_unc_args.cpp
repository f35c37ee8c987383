// AddressSanitizer run of the HOST side of libpacingpseudo_unc (include/pacingpseudo_unc.h): the argument checks of every
// punc_* entry point, built for the host only (`make asan-unc`, no GPU needed).  Every call below must be rejected BEFORE
// anything is launched: return code < 0 (0 bytes from the size query), a message in punc_last_error(), no out-of-bounds access
// while the check builds its message.
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "pacingpseudo_unc.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                              \
  do {                                                                                   \
    const int rc = (call);                                                               \
    const char* msg = punc_last_error();                                                 \
    if (rc >= 0 || !msg || !msg[0]) { printf("NOT REJECTED: %s -> %d\n", #call, rc); ++failures; } \
  } while (0)
#define EXPECT_ZERO_BYTES(call)                                                          \
  do {                                                                                   \
    const size_t nb = (call);                                                            \
    if (nb != 0) { printf("NOT REJECTED: %s -> %zu bytes\n", #call, nb); ++failures; }   \
  } while (0)

int main() {
  if (punc_version() < 100) ++failures;
  if (!punc_last_error()) ++failures;

  // host memory standing in for device buffers: nothing may be launched, so nothing dereferences them on a device
  alignas(256) static float img[64], out[64], z[5 * 64], acc[5 * 64], mask[64], unc[64], valid[64];
  alignas(256) static double stats[3], wsbuf[64];
  alignas(256) static unsigned long long state[2] = {1ull, 0ull};
  void* ws = wsbuf;
  const size_t nb = sizeof(wsbuf);

  // size query
  EXPECT_ZERO_BYTES(punc_workspace_bytes(0, 5, 64));
  EXPECT_ZERO_BYTES(punc_workspace_bytes(-2, 5, 64));
  EXPECT_ZERO_BYTES(punc_workspace_bytes(1, 1, 64));
  EXPECT_ZERO_BYTES(punc_workspace_bytes(1, 33, 64));
  EXPECT_ZERO_BYTES(punc_workspace_bytes(1, 5, 0));
  EXPECT_ZERO_BYTES(punc_workspace_bytes(65536, 5, 65536));          // N * HW >= 2^31
  if (punc_workspace_bytes(1, 5, 64) != 3 * sizeof(double)) { printf("one block of pixels needs three doubles\n"); ++failures; }
  if (punc_workspace_bytes(2, 5, 300) != 3 * 3 * sizeof(double)) { printf("600 pixels are three blocks\n"); ++failures; }

  // noise: null pointers, alignment, sizes, parameters, pass
  EXPECT_REJECT(punc_noise_add(nullptr, 64, 0.1f, 0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, 0.1f, 0.2f, nullptr, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, 0.1f, 0.2f, state, 0, nullptr, nullptr));
  EXPECT_REJECT(punc_noise_add((const float*)((const char*)img + 2), 60, 0.1f, 0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, 0.1f, 0.2f, (const unsigned long long*)((const char*)state + 4), 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 0, 0.1f, 0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, -4, 0.1f, 0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, (1ll << 34) + 1, 0.1f, 0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, -0.1f, 0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, NAN, 0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, INFINITY, 0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, 0.1f, -0.2f, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, 0.1f, NAN, state, 0, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, 0.1f, 0.2f, state, -1, out, nullptr));
  EXPECT_REJECT(punc_noise_add(img, 64, 0.1f, 0.2f, state, 16, out, nullptr));

  // accumulate: null pointers, one at a time (valid_mask and unc may be null)
  EXPECT_REJECT(punc_accumulate(nullptr, 1, 5, 64, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, 1.f, nullptr, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, 1.f, acc, nullptr, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, 1.f, acc, mask, unc, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, 1.f, acc, mask, unc, stats, nullptr, nb, nullptr));
  // alignment
  EXPECT_REJECT(punc_accumulate((const float*)((const char*)z + 2), 1, 5, 60, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, 1.f, acc, mask, unc, (double*)((char*)stats + 4), ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, 1.f, acc, mask, unc, stats, (char*)ws + 4, nb - 4, nullptr));
  // shapes
  EXPECT_REJECT(punc_accumulate(z, 0, 5, 64, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 1, 64, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 0, 64, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 33, 64, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 0, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 65536, 5, 65536, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  // passes
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 0, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 17, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 1, 1, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 4, 4, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, -1, 4, valid, 1.f, acc, mask, unc, stats, ws, nb, nullptr));
  // threshold
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, NAN, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, INFINITY, acc, mask, unc, stats, ws, nb, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, -INFINITY, acc, mask, unc, stats, ws, nb, nullptr));
  // workspace too small (also on a pass that would not use it)
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 1, valid, 1.f, acc, mask, unc, stats, ws, 3 * sizeof(double) - 1, nullptr));
  EXPECT_REJECT(punc_accumulate(z, 1, 5, 64, 0, 3, nullptr, 1.f, acc, mask, nullptr, stats, ws, 0, nullptr));

  // advance
  EXPECT_REJECT(punc_advance(nullptr, nullptr));
  EXPECT_REJECT(punc_advance((unsigned long long*)((char*)state + 4), nullptr));

  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("asan_unc_args: all argument checks rejected their input, no sanitizer report\n");
  return 0;
}
