// AddressSanitizer run of the HOST side of libpacingpseudo_geo (include/pacingpseudo_geo.h): the argument checks of every
// pgeo_* entry point, built for the host only (`make asan-geo`, no GPU needed).  Every call below must be rejected BEFORE
// anything is launched: return code < 0 (0 bytes from the size query), a message in pgeo_last_error(), no out-of-bounds access
// while the check reads the table of sizes or builds its message.
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "pacingpseudo_geo.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                              \
  do {                                                                                   \
    const int rc = (call);                                                               \
    const char* msg = pgeo_last_error();                                                 \
    if (rc >= 0 || !msg || !msg[0]) { printf("NOT REJECTED: %s -> %d\n", #call, rc); ++failures; } \
  } while (0)
#define EXPECT_ZERO_BYTES(call)                                                          \
  do {                                                                                   \
    const size_t nb = (call);                                                            \
    if (nb != 0) { printf("NOT REJECTED: %s -> %zu bytes\n", #call, nb); ++failures; }   \
  } while (0)

int main() {
  if (pgeo_version() < 100) ++failures;
  if (!pgeo_last_error()) ++failures;

  // host memory standing in for device buffers: nothing may be launched, so nothing dereferences them on a device
  alignas(256) static float img[2 * 64], g[2 * 64], dist[2 * 5 * 64];
  alignas(256) static int scb[2 * 64], out[2 * 64], stats[2 * 5 * 2];
  alignas(256) static double wsbuf[16];
  void* ws = wsbuf;
  const size_t nb = sizeof(wsbuf);
  static const int ok_sizes[4] = {8, 8, 5, 3};
  static const int tall[4] = {8, 8, 9, 3}, wide[4] = {8, 8, 5, 9}, zero_h[4] = {0, 8, 5, 3}, neg_w[4] = {8, 8, 5, -1};

  // size query
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(0, 5, 8, 8));
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(-1, 5, 8, 8));
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(1, 0, 8, 8));
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(1, 33, 8, 8));
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(1, 5, 0, 8));
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(1, 5, 8, 0));
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(1, 5, 1025, 8));
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(1, 5, 8, 1025));
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(64, 32, 1024, 1024));          // N * K * H * W = 2^31
  EXPECT_ZERO_BYTES(pgeo_distance_workspace(2147483647, 32, 1024, 1024));
  if (pgeo_distance_workspace(1, 1, 8, 8) != 8) { printf("one tile: 1 byte rounded up to 8\n"); ++failures; }
  if (pgeo_distance_workspace(2, 5, 65, 129) != 64) { printf("2 x 5 planes of 2 x 3 tiles need 60 bytes, rounded up to 64\n"); ++failures; }
  if (pgeo_distance_workspace(63, 32, 1024, 1024) != 63u * 32u * 256u) { printf("the largest batch\n"); ++failures; }

  // normalize: null pointers, alignment, shapes, sizes
  EXPECT_REJECT(pgeo_normalize(nullptr, nullptr, 2, 8, 8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, nullptr, 2, 8, 8, nullptr, nullptr));
  EXPECT_REJECT(pgeo_normalize((const float*)((const char*)img + 2), nullptr, 1, 8, 8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, nullptr, 2, 8, 8, (float*)((char*)g + 1), nullptr));
  EXPECT_REJECT(pgeo_normalize(img, nullptr, 0, 8, 8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, nullptr, 2, 0, 8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, nullptr, 2, 8, -8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, nullptr, 2, 1025, 8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, nullptr, 2048, 1024, 1024, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, tall, 2, 8, 8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, wide, 2, 8, 8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, zero_h, 2, 8, 8, g, nullptr));
  EXPECT_REJECT(pgeo_normalize(img, neg_w, 2, 8, 8, g, nullptr));

  // distance
  EXPECT_REJECT(pgeo_distance(nullptr, scb, ok_sizes, 2, 5, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, nullptr, ok_sizes, 2, 5, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, ok_sizes, 2, 5, 8, 8, 20.f, 100, nullptr, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, ok_sizes, 2, 5, 8, 8, 20.f, 100, dist, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, ok_sizes, 2, 5, 8, 8, 20.f, 100, dist, stats, nullptr, nb, nullptr));
  EXPECT_REJECT(pgeo_distance((const float*)((const char*)g + 2), scb, nullptr, 1, 5, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, (const int*)((const char*)scb + 1), nullptr, 1, 5, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 8, 20.f, 100, (float*)((char*)dist + 2), stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 8, 20.f, 100, dist, (int*)((char*)stats + 2), ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 8, 20.f, 100, dist, stats, (char*)ws + 4, nb - 4, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 8, -1.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 8, NAN, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 8, INFINITY, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 8, 20.f, 0, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 8, 20.f, -5, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 0, 5, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 0, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 33, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 0, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 2, 5, 8, 1025, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, nullptr, 64, 32, 1024, 1024, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, tall, 2, 5, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, neg_w, 2, 5, 8, 8, 20.f, 100, dist, stats, ws, nb, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, ok_sizes, 2, 5, 8, 8, 20.f, 100, dist, stats, ws, 15, nullptr));
  EXPECT_REJECT(pgeo_distance(g, scb, ok_sizes, 2, 5, 8, 8, 20.f, 100, dist, stats, ws, 0, nullptr));

  // labels
  EXPECT_REJECT(pgeo_labels(nullptr, scb, ok_sizes, 2, 5, 8, 8, INFINITY, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, nullptr, ok_sizes, 2, 5, 8, 8, INFINITY, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, ok_sizes, 2, 5, 8, 8, INFINITY, 0.25f, nullptr, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 5, 8, 8, INFINITY, 0.25f, (int*)((char*)out + 2), nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 5, 8, 8, 0.f, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 5, 8, 8, -1.f, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 5, 8, 8, NAN, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 5, 8, 8, INFINITY, 0.f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 5, 8, 8, INFINITY, 1.5f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 5, 8, 8, INFINITY, NAN, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 0, 5, 8, 8, INFINITY, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 33, 8, 8, INFINITY, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, nullptr, 2, 5, 1025, 8, INFINITY, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, wide, 2, 5, 8, 8, INFINITY, 0.25f, out, nullptr));
  EXPECT_REJECT(pgeo_labels(dist, scb, zero_h, 2, 5, 8, 8, INFINITY, 0.25f, out, nullptr));

  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("asan_geo_args: all argument checks rejected their input, no sanitizer report\n");
  return 0;
}
