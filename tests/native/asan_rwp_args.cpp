// AddressSanitizer run of the HOST side of libpacingpseudo_rwp (include/pacingpseudo_rwp.h): the argument checks of every
// prwp_* entry point, built for the host only (`make asan-rwp`, no GPU needed).  Every call below must be rejected BEFORE
// anything is launched: return code < 0 (0 bytes from the size query), a message in prwp_last_error(), no out-of-bounds access
// while the check reads `sizes` or builds its message.
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "pacingpseudo_rwp.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                              \
  do {                                                                                   \
    const int rc = (call);                                                               \
    const char* msg = prwp_last_error();                                                 \
    if (rc >= 0 || !msg || !msg[0]) { printf("NOT REJECTED: %s -> %d\n", #call, rc); ++failures; } \
  } while (0)
#define EXPECT_ZERO_BYTES(call)                                                          \
  do {                                                                                   \
    const size_t nb = (call);                                                            \
    if (nb != 0) { printf("NOT REJECTED: %s -> %zu bytes\n", #call, nb); ++failures; }   \
  } while (0)

int main() {
  if (prwp_version() < 100) ++failures;
  if (!prwp_last_error()) ++failures;

  // host memory standing in for device buffers: nothing may be launched, so nothing dereferences them on a device
  alignas(256) static float img[64], z[5 * 64], prob[5 * 64], stats[15], wsbuf[4096];
  alignas(256) static int scb[64];
  void* ws = wsbuf;
  std::vector<int> ok = {8, 8}, tall = {9, 8}, wide = {8, 9}, zero = {0, 8}, neg = {8, -1};
  std::vector<int> second_bad = {8, 8, 8, 8, 100, 8};          // exactly N pairs on the heap: one read further is a report

  // size query
  EXPECT_ZERO_BYTES(prwp_workspace_bytes(0, 5, 8, 8));
  EXPECT_ZERO_BYTES(prwp_workspace_bytes(1, 0, 8, 8));
  EXPECT_ZERO_BYTES(prwp_workspace_bytes(1, 33, 8, 8));
  EXPECT_ZERO_BYTES(prwp_workspace_bytes(1, 5, 0, 8));
  EXPECT_ZERO_BYTES(prwp_workspace_bytes(1, 5, 8, 1025));
  EXPECT_ZERO_BYTES(prwp_workspace_bytes(-3, 5, 8, 8));
  if (prwp_workspace_bytes(1, 5, 8, 8) < (size_t)(3 + 15) * 64 * sizeof(float)) { printf("workspace too small for its planes\n"); ++failures; }
  if (prwp_workspace_bytes(64, 32, 1024, 1024) <= ((size_t)1 << 32)) { printf("workspace size wrapped at 32 bits\n"); ++failures; }

  // solve: null pointers, one at a time
  EXPECT_REJECT(prwp_solve(nullptr, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, nullptr, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, nullptr, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, nullptr, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, nullptr, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, nullptr, nullptr));
  // alignment
  EXPECT_REJECT(prwp_solve(img, scb, (const float*)((const char*)z + 2), ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, (char*)ws + 16, nullptr));
  // shapes
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 0, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 0, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 33, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 0, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, nullptr, 1, 5, 1025, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, tall.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));      // h > H
  EXPECT_REJECT(prwp_solve(img, scb, z, wide.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));      // w > W
  EXPECT_REJECT(prwp_solve(img, scb, z, zero.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, neg.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, second_bad.data(), 3, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  // parameters
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, -1.f, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, NAN, 1e-4f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 0.f, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, INFINITY, 0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, -0.1f, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, NAN, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, INFINITY, 1e-6f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 0.f, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, NAN, 100, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, 0, prob, stats, ws, nullptr));
  EXPECT_REJECT(prwp_solve(img, scb, z, ok.data(), 1, 5, 8, 8, 13.f, 1e-4f, 0.1f, 1e-6f, -5, prob, stats, ws, nullptr));

  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("asan_rwp_args: all argument checks rejected their input, no sanitizer report\n");
  return 0;
}
