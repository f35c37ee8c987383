// AddressSanitizer run of the HOST side of libpacingpseudo_dist (include/pacingpseudo_dist.h): the argument checks of every
// pdist_* entry point, built for the host only (`make asan-dist`, no GPU needed).  Every call below must be rejected BEFORE
// anything is launched: return code < 0 (0 bytes from a size query), a message in pdist_last_error(), no out-of-bounds access
// while the check builds its message.
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "pacingpseudo_dist.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                              \
  do {                                                                                   \
    const int rc = (call);                                                               \
    const char* msg = pdist_last_error();                                                \
    if (rc >= 0 || !msg || !msg[0]) { printf("NOT REJECTED: %s -> %d\n", #call, rc); ++failures; } \
  } while (0)
#define EXPECT_ZERO_BYTES(call)                                                          \
  do {                                                                                   \
    const size_t nb = (call);                                                            \
    if (nb != 0) { printf("NOT REJECTED: %s -> %zu bytes\n", #call, nb); ++failures; }   \
  } while (0)

int main() {
  if (pdist_version() < 100) ++failures;
  if (!pdist_last_error()) ++failures;

  // host memory standing in for device buffers: nothing may be launched, so nothing dereferences them on a device
  alignas(256) static unsigned char mask[64];
  alignas(256) static long long cls[64];
  alignas(256) static float out[64], z[5 * 64], phi[5 * 64], dz[5 * 64], loss[1], grad[1];
  alignas(256) static double wsbuf[128];
  void* ws = wsbuf;
  const size_t nb = sizeof(wsbuf);

  // size queries
  EXPECT_ZERO_BYTES(pdist_edt_workspace(0, 8, 8));
  EXPECT_ZERO_BYTES(pdist_edt_workspace(-1, 8, 8));
  EXPECT_ZERO_BYTES(pdist_edt_workspace(1, 0, 8));
  EXPECT_ZERO_BYTES(pdist_edt_workspace(1, 8, 0));
  EXPECT_ZERO_BYTES(pdist_edt_workspace(1, 2049, 8));
  EXPECT_ZERO_BYTES(pdist_edt_workspace(1, 8, 2049));
  EXPECT_ZERO_BYTES(pdist_edt_workspace(512, 2048, 2048));           // P * H * W = 2^31
  EXPECT_ZERO_BYTES(pdist_signed_maps_workspace(0, 5, 8, 8));
  EXPECT_ZERO_BYTES(pdist_signed_maps_workspace(1, 0, 8, 8));
  EXPECT_ZERO_BYTES(pdist_signed_maps_workspace(1, 33, 8, 8));
  EXPECT_ZERO_BYTES(pdist_signed_maps_workspace(1, 5, 2049, 8));
  EXPECT_ZERO_BYTES(pdist_signed_maps_workspace(16, 32, 2048, 2048));      // N * K * H * W = 2^31
  EXPECT_ZERO_BYTES(pdist_signed_maps_workspace(2147483647, 32, 2048, 2048));
  EXPECT_ZERO_BYTES(pdist_boundary_loss_workspace(0, 5, 8, 8));
  EXPECT_ZERO_BYTES(pdist_boundary_loss_workspace(1, 33, 8, 8));
  EXPECT_ZERO_BYTES(pdist_boundary_loss_workspace(1, 5, 8, 4096));
  if (pdist_edt_workspace(1, 8, 8) != 128) { printf("64 pixels need 128 bytes\n"); ++failures; }
  if (pdist_edt_workspace(1, 1, 1) != 8) { printf("one pixel: 2 bytes rounded up to 8\n"); ++failures; }
  if (pdist_signed_maps_workspace(1, 5, 8, 8) != 640) { printf("5 x 64 pixels need 640 bytes\n"); ++failures; }
  if (pdist_boundary_loss_workspace(2, 5, 10, 30) != 3 * sizeof(double)) { printf("600 pixels are three blocks\n"); ++failures; }

  // edt: null pointers, alignment, shapes, spacing, flag, workspace
  EXPECT_REJECT(pdist_edt(nullptr, 1, 8, 8, 1.f, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, 1.f, 0, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, 1.f, 0, out, nullptr, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, 1.f, 0, (float*)((char*)out + 2), ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, 1.f, 0, out, (char*)ws + 4, nb - 4, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 0, 8, 8, 1.f, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 0, 8, 1.f, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, -8, 1.f, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 2049, 1, 1.f, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 1, 2049, 1.f, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 512, 2048, 2048, 1.f, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 0.f, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, -1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, NAN, 1.f, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, INFINITY, 0, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, 1.f, 2, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, 1.f, -1, out, ws, nb, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, 1.f, 0, out, ws, 127, nullptr));
  EXPECT_REJECT(pdist_edt(mask, 1, 8, 8, 1.f, 1.f, 0, out, ws, 0, nullptr));

  // signed maps
  EXPECT_REJECT(pdist_signed_maps(nullptr, 1, 5, 8, 8, 1.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 8, 1.f, 1.f, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 8, 1.f, 1.f, phi, nullptr, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps((const long long*)((const char*)cls + 4), 1, 5, 7, 8, 1.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 8, 1.f, 1.f, (float*)((char*)phi + 2), ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 8, 1.f, 1.f, phi, (char*)ws + 4, nb - 4, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 0, 5, 8, 8, 1.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 0, 8, 8, 1.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 33, 8, 8, 1.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 0, 8, 1.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 2049, 1.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 16, 32, 2048, 2048, 1.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 8, 0.f, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 8, 1.f, NAN, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 8, -INFINITY, 1.f, phi, ws, nb, nullptr));
  EXPECT_REJECT(pdist_signed_maps(cls, 1, 5, 8, 8, 1.f, 1.f, phi, ws, 639, nullptr));

  // loss forward
  EXPECT_REJECT(pdist_boundary_loss_fwd(nullptr, phi, 1, 5, 8, 8, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, nullptr, 1, 5, 8, 8, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 1, 5, 8, 8, nullptr, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 1, 5, 8, 8, loss, nullptr, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd((const float*)((const char*)z + 2), phi, 1, 5, 7, 8, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 1, 5, 8, 8, loss, (char*)ws + 4, nb - 4, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 0, 5, 8, 8, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 1, 0, 8, 8, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 1, 33, 8, 8, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 1, 5, 0, 8, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 1, 5, 8, 4096, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 16, 32, 2048, 2048, loss, ws, nb, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_fwd(z, phi, 1, 5, 8, 8, loss, ws, 7, nullptr));

  // loss backward
  EXPECT_REJECT(pdist_boundary_loss_bwd(nullptr, phi, 1, 5, 8, 8, grad, dz, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, nullptr, 1, 5, 8, 8, grad, dz, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 1, 5, 8, 8, nullptr, dz, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 1, 5, 8, 8, grad, nullptr, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 1, 5, 8, 8, grad, (float*)((char*)dz + 2), nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 0, 5, 8, 8, grad, dz, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 1, 0, 8, 8, grad, dz, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 1, 33, 8, 8, grad, dz, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 1, 5, 2049, 8, grad, dz, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 1, 5, 8, 0, grad, dz, nullptr));
  EXPECT_REJECT(pdist_boundary_loss_bwd(z, phi, 16, 32, 2048, 2048, grad, dz, nullptr));

  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("asan_dist_args: all argument checks rejected their input, no sanitizer report\n");
  return 0;
}
