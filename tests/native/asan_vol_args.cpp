// AddressSanitizer run of the HOST side of libpacingpseudo_vol (include/pacingpseudo_vol.h): the argument checks of every
// pvol_* entry point, built for the host only (`make asan-vol`, no GPU needed).  Every call below must be rejected BEFORE
// anything is launched: return code < 0 (0 bytes from a size query), a message in pvol_last_error(), no out-of-bounds access
// while the check builds its message.
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "pacingpseudo_vol.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                              \
  do {                                                                                   \
    const int rc = (call);                                                               \
    const char* msg = pvol_last_error();                                                 \
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
  if (pvol_version() < 100) ++failures;
  if (!pvol_last_error()) ++failures;

  // host memory standing in for device buffers: nothing may be launched, so nothing dereferences them on a device
  alignas(256) static int64_t cls[2 * 64], lab[2 * 64], out[2 * 64];
  alignas(256) static int32_t labels[2 * 64], stats[32 * 2], counts[32 * 4];
  alignas(256) static float field[2 * 64], dist[5 * 2 * 128];
  alignas(256) static unsigned char mask[2 * 64];
  alignas(256) static double wsbuf[1024];
  void* ws = wsbuf;
  const size_t nb = sizeof(wsbuf);
  char* odd = (char*)ws + 4;

  // size queries: the formulas of the header, and 0 for what the calls refuse
  EXPECT_BYTES(pvol_label_workspace(2, 8, 8), 512);
  EXPECT_BYTES(pvol_label_workspace(1, 1, 1), 8);
  EXPECT_BYTES(pvol_keep_largest_workspace(5, 2, 8, 8), 80 + 3 * 512);
  EXPECT_BYTES(pvol_edt_workspace(3, 3, 3), 56);
  EXPECT_BYTES(pvol_surface_workspace(5, 2, 8, 8), 512 + 256 + 2 * 128 + 24);
  EXPECT_BYTES(pvol_surface_workspace(4, 2, 64, 33), 4 * 4224 + 2 * 4224 + 2 * 4224 + 48);
  EXPECT_ZERO_BYTES(pvol_label_workspace(0, 8, 8));
  EXPECT_ZERO_BYTES(pvol_label_workspace(-1, 8, 8));
  EXPECT_ZERO_BYTES(pvol_label_workspace(4097, 8, 8));
  EXPECT_ZERO_BYTES(pvol_label_workspace(2, 0, 8));
  EXPECT_ZERO_BYTES(pvol_label_workspace(2, 8, 2049));
  EXPECT_ZERO_BYTES(pvol_label_workspace(512, 2048, 2048));            // D * H * W = 2^31
  EXPECT_ZERO_BYTES(pvol_label_workspace(4096, 2048, 2048));
  EXPECT_ZERO_BYTES(pvol_keep_largest_workspace(0, 2, 8, 8));
  EXPECT_ZERO_BYTES(pvol_keep_largest_workspace(33, 2, 8, 8));
  EXPECT_ZERO_BYTES(pvol_keep_largest_workspace(5, 2, 8, -8));
  EXPECT_ZERO_BYTES(pvol_edt_workspace(2, 2049, 8));
  EXPECT_ZERO_BYTES(pvol_edt_workspace(0, 8, 8));
  EXPECT_ZERO_BYTES(pvol_surface_workspace(0, 2, 8, 8));
  EXPECT_ZERO_BYTES(pvol_surface_workspace(33, 2, 8, 8));
  EXPECT_ZERO_BYTES(pvol_surface_workspace(5, 2, 0, 8));
  EXPECT_ZERO_BYTES(pvol_surface_workspace(32, 8, 2048, 2048));        // K * 2 * D * H * W = 2^31

  // label_components
  EXPECT_REJECT(pvol_label_components(nullptr, 2, 8, 8, 1, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, 1, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, 1, labels, nullptr, nb, nullptr));
  EXPECT_REJECT(pvol_label_components((const int64_t*)((const char*)cls + 4), 1, 8, 8, 1, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, 1, (int32_t*)((char*)labels + 2), ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, 1, labels, odd, nb - 4, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 0, 8, 8, 1, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 4097, 8, 8, 1, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 0, 8, 1, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 2049, 1, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 512, 2048, 2048, 1, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, 0, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, 4, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, -1, labels, ws, nb, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, 1, labels, ws, 511, nullptr));
  EXPECT_REJECT(pvol_label_components(cls, 2, 8, 8, 1, labels, ws, 0, nullptr));

  // keep_largest_components
  EXPECT_REJECT(pvol_keep_largest_components(nullptr, 5, 2, 8, 8, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 1, nullptr, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 1, out, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 1, out, stats, nullptr, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 1, (int64_t*)((char*)out + 4), stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 1, out, (int32_t*)((char*)stats + 1), ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 1, out, stats, odd, nb - 4, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 0, 2, 8, 8, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 33, 2, 8, 8, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 0, 8, 8, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 2049, 8, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, -3, 1, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 0, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 4, out, stats, ws, nb, nullptr));
  EXPECT_REJECT(pvol_keep_largest_components(cls, 5, 2, 8, 8, 1, out, stats, ws, 80 + 3 * 512 - 1, nullptr));

  // edt
  EXPECT_REJECT(pvol_edt(nullptr, 2, 8, 8, 1.f, 1.f, 1.f, 0, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, 1.f, 1.f, 0, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, 1.f, 1.f, 0, field, nullptr, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, 1.f, 1.f, 0, (float*)((char*)field + 2), ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, 1.f, 1.f, 0, field, odd, nb - 4, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 0, 8, 8, 1.f, 1.f, 1.f, 0, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 4097, 8, 8, 1.f, 1.f, 1.f, 0, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 2049, 1.f, 1.f, 1.f, 0, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 0.f, 1.f, 1.f, 0, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, -1.f, 1.f, 0, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, 1.f, NAN, 0, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, INFINITY, 1.f, 1.f, 0, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, 1.f, 1.f, 2, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, 1.f, 1.f, -1, field, ws, nb, nullptr));
  EXPECT_REJECT(pvol_edt(mask, 2, 8, 8, 1.f, 1.f, 1.f, 0, field, ws, 255, nullptr));

  // surface_distances
  EXPECT_REJECT(pvol_surface_distances(nullptr, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, nullptr, 5, 2, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, nullptr, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, dist, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, dist, counts, nullptr, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances((const int64_t*)((const char*)cls + 4), lab, 5, 1, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, (const int64_t*)((const char*)lab + 2), 5, 1, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, (float*)((char*)dist + 1), counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, dist, (int32_t*)((char*)counts + 2), ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, dist, counts, odd, nb - 4, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 0, 2, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 33, 2, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 0, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 2049, 8, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 32, 8, 2048, 2048, 1.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 0.f, 1.f, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, NAN, 1.f, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, -INFINITY, dist, counts, ws, nb, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, 512 + 256 + 2 * 128 + 24 - 1, nullptr));
  EXPECT_REJECT(pvol_surface_distances(cls, lab, 5, 2, 8, 8, 1.f, 1.f, 1.f, dist, counts, ws, 0, nullptr));

  // dice_counts
  EXPECT_REJECT(pvol_dice_counts(nullptr, lab, 5, 2, 8, 8, counts, nullptr));
  EXPECT_REJECT(pvol_dice_counts(cls, nullptr, 5, 2, 8, 8, counts, nullptr));
  EXPECT_REJECT(pvol_dice_counts(cls, lab, 5, 2, 8, 8, nullptr, nullptr));
  EXPECT_REJECT(pvol_dice_counts((const int64_t*)((const char*)cls + 4), lab, 5, 1, 8, 8, counts, nullptr));
  EXPECT_REJECT(pvol_dice_counts(cls, lab, 5, 2, 8, 8, (int32_t*)((char*)counts + 2), nullptr));
  EXPECT_REJECT(pvol_dice_counts(cls, lab, 0, 2, 8, 8, counts, nullptr));
  EXPECT_REJECT(pvol_dice_counts(cls, lab, 33, 2, 8, 8, counts, nullptr));
  EXPECT_REJECT(pvol_dice_counts(cls, lab, 5, 0, 8, 8, counts, nullptr));
  EXPECT_REJECT(pvol_dice_counts(cls, lab, 5, 2, 8, 2049, counts, nullptr));
  EXPECT_REJECT(pvol_dice_counts(cls, lab, 5, 512, 2048, 2048, counts, nullptr));

  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("asan_vol_args: all argument checks rejected their input, no sanitizer report\n");
  return 0;
}
