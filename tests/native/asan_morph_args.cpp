// AddressSanitizer run of the HOST side of libpacingpseudo_morph (include/pacingpseudo_morph.h): the argument checks of every
// pmor_* entry point, built for the host only (`make asan-morph`, no GPU needed).  Every call below must be rejected BEFORE
// anything is launched: return code < 0 (0 bytes from the size query), a message in pmor_last_error(), no out-of-bounds access
// while the check builds its message.
#include <stdio.h>
#include <string.h>
#include "pacingpseudo_morph.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                              \
  do {                                                                                   \
    const int rc = (call);                                                               \
    const char* msg = pmor_last_error();                                                 \
    if (rc >= 0 || !msg || !msg[0]) { printf("NOT REJECTED: %s -> %d\n", #call, rc); ++failures; } \
  } while (0)
#define EXPECT_ZERO_BYTES(call)                                                          \
  do {                                                                                   \
    const size_t nb = (call);                                                            \
    if (nb != 0) { printf("NOT REJECTED: %s -> %zu bytes\n", #call, nb); ++failures; }   \
  } while (0)
#define EXPECT_BYTES(call, want)                                                         \
  do {                                                                                   \
    const size_t nb = (call);                                                            \
    if (nb != (size_t)(want)) { printf("%s -> %zu bytes, expected %zu\n", #call, nb, (size_t)(want)); ++failures; } \
  } while (0)

int main() {
  if (pmor_version() < 100) ++failures;
  if (!pmor_last_error()) ++failures;

  // host memory standing in for device buffers: nothing may be launched, so nothing dereferences them on a device
  alignas(256) static int64_t cls[2 * 64], out[2 * 64];
  alignas(256) static int32_t labels[2 * 64], stats[2 * 32 * 2];
  alignas(256) static double wsbuf[1024];
  static const int32_t min_size[32] = {0, 5, 5, 5, 5};
  void* ws = wsbuf;
  const size_t nb = sizeof(wsbuf);
  char* odd = (char*)ws + 4;

  // the size query: the formula of the header, and 0 for what the calls refuse
  EXPECT_BYTES(pmor_workspace(2, 5, 1, 8, 8, 2), 512);
  EXPECT_BYTES(pmor_workspace(1, 5, 2, 8, 8, 3), 512);
  EXPECT_BYTES(pmor_workspace(1, 1, 1, 1, 1, 2), 8);
  EXPECT_BYTES(pmor_workspace(3, 32, 1, 1, 1, 3), 16);
  EXPECT_ZERO_BYTES(pmor_workspace(0, 5, 1, 8, 8, 2));
  EXPECT_ZERO_BYTES(pmor_workspace(-1, 5, 1, 8, 8, 2));
  EXPECT_ZERO_BYTES(pmor_workspace(2, 0, 1, 8, 8, 2));
  EXPECT_ZERO_BYTES(pmor_workspace(2, 33, 1, 8, 8, 2));
  EXPECT_ZERO_BYTES(pmor_workspace(2, 5, 2, 8, 8, 2));                 // a slice has D = 1
  EXPECT_ZERO_BYTES(pmor_workspace(2, 5, 0, 8, 8, 3));
  EXPECT_ZERO_BYTES(pmor_workspace(1, 5, 4097, 8, 8, 3));
  EXPECT_ZERO_BYTES(pmor_workspace(2, 5, 1, 0, 8, 2));
  EXPECT_ZERO_BYTES(pmor_workspace(2, 5, 1, 8, 2049, 2));
  EXPECT_ZERO_BYTES(pmor_workspace(2, 5, 1, 8, 8, 1));
  EXPECT_ZERO_BYTES(pmor_workspace(2, 5, 1, 8, 8, 4));
  EXPECT_ZERO_BYTES(pmor_workspace(1, 5, 512, 2048, 2048, 3));         // D * H * W = 2^31
  EXPECT_ZERO_BYTES(pmor_workspace(512, 5, 1, 2048, 2048, 2));         // N * H * W = 2^31
  EXPECT_ZERO_BYTES(pmor_workspace(2147483647, 5, 1, 2048, 2048, 2));

  // remove_small
  EXPECT_REJECT(pmor_remove_small(nullptr, labels, 2, 5, 1, 8, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, nullptr, 2, 5, 1, 8, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 8, 2, nullptr, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 8, 2, min_size, nullptr, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 8, 2, min_size, out, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 8, 2, min_size, out, stats, nullptr, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small((const int64_t*)((const char*)cls + 4), labels, 1, 5, 1, 8, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, (const int32_t*)((const char*)labels + 2), 1, 5, 1, 8, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 1, 5, 1, 8, 8, 2, min_size, (int64_t*)((char*)out + 4), stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 1, 5, 1, 8, 8, 2, min_size, out, (int32_t*)((char*)stats + 1), ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 1, 5, 1, 8, 8, 2, min_size, out, stats, odd, nb - 4, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 0, 5, 1, 8, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 0, 1, 8, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 33, 1, 8, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 1, 5, 2, 8, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 1, 5, 0, 8, 8, 3, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 1, 5, 4097, 8, 8, 3, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 0, 8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 2049, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, -8, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 8, 0, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 8, 4, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 1, 5, 512, 2048, 2048, 3, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 512, 5, 1, 2048, 2048, 2, min_size, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 8, 2, min_size, out, stats, ws, 511, nullptr));
  EXPECT_REJECT(pmor_remove_small(cls, labels, 2, 5, 1, 8, 8, 2, min_size, out, stats, ws, 0, nullptr));

  // fill_holes
  EXPECT_REJECT(pmor_fill_holes(nullptr, labels, 2, 5, 1, 8, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, nullptr, 2, 5, 1, 8, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 8, 8, 2, 1, nullptr, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 8, 8, 2, 1, out, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 8, 8, 2, 1, out, stats, nullptr, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes((const int64_t*)((const char*)cls + 4), labels, 1, 5, 1, 8, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, (const int32_t*)((const char*)labels + 2), 1, 5, 1, 8, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 1, 8, 8, 2, 1, (int64_t*)((char*)out + 4), stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 1, 8, 8, 2, 1, out, (int32_t*)((char*)stats + 2), ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 1, 8, 8, 2, 1, out, stats, odd, nb - 4, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 0, 5, 1, 8, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 0, 1, 8, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 33, 1, 8, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 2, 8, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 4097, 8, 8, 3, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 2049, 8, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 8, 0, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 8, 8, 5, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 8, 8, 2, 0, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 8, 8, 2, 3, out, stats, ws, nb, nullptr));          // 2-D: 1 or 2
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 2, 8, 8, 3, 4, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 2, 8, 8, 3, -1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 512, 2048, 2048, 3, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 512, 5, 1, 2048, 2048, 2, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 2, 5, 1, 8, 8, 2, 1, out, stats, ws, 511, nullptr));
  EXPECT_REJECT(pmor_fill_holes(cls, labels, 1, 5, 2, 8, 8, 3, 1, out, stats, ws, 0, nullptr));

  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("asan_morph_args: all argument checks rejected their input, no sanitizer report\n");
  return 0;
}
