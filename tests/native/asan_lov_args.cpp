// AddressSanitizer run of the HOST side of libpacingpseudo_lov (include/pacingpseudo_lov.h): the argument checks of every
// plov_* entry point, built for the host only (`make asan-lov`, no GPU needed).  Every call below must be rejected BEFORE
// anything is launched: return code < 0 (size queries: 0), a message in plov_last_error(), no out-of-bounds access while the check
// builds its message.
#include <stdio.h>
#include <string.h>
#include "pacingpseudo_lov.h"

static int failures = 0;
#define EXPECT_REJECT(call)                                                              \
  do {                                                                                   \
    const int rc = (call);                                                               \
    const char* msg = plov_last_error();                                                 \
    if (rc >= 0 || !msg || !msg[0]) { printf("NOT REJECTED: %s -> %d\n", #call, rc); ++failures; } \
  } while (0)
#define EXPECT_ZERO(call)                                                                \
  do {                                                                                   \
    const size_t b = (call);                                                             \
    if (b != 0) { printf("NOT REFUSED: %s -> %zu\n", #call, b); ++failures; }            \
  } while (0)

// host memory standing in for device buffers: nothing may be launched, so nothing dereferences them on a device
alignas(256) static float z[256], out[256], w[256], sc[64], err[256], up[4], loss[4];
alignas(256) static long long t[64];
alignas(256) static int perm[256];
alignas(256) static char ws[1 << 16];

static float* off(float* a, int bytes) { return (float*)((char*)a + bytes); }

static int fwd(const float* z_, const long long* t_, int N, int K, int H, int W, float* loss_, float* w_, float* sc_, float* err_, int* perm_,
               void* ws_, size_t bytes, int has_ignore = 1, int per_image = 0, int classes_all = 0) {
  return plov_loss_fwd(z_, t_, N, K, H, W, has_ignore, 5, per_image, classes_all, loss_, w_, sc_, err_, perm_, ws_, bytes, nullptr);
}

static int bwd(const float* z_, const long long* t_, int N, int K, int H, int W, const float* w_, const float* sc_, const float* up_,
               float* dz_, int has_ignore = 1, int per_image = 0) {
  return plov_loss_bwd(z_, t_, N, K, H, W, has_ignore, 5, per_image, w_, sc_, up_, dz_, nullptr);
}

int main() {
  if (plov_version() < 100) ++failures;
  if (!plov_last_error()) ++failures;
  if (plov_tile() < 64) { printf("plov_tile: at least one wave of keys\n"); ++failures; }

  // ---- the sort
  const size_t sb = plov_sort_workspace(2, 8);
  if (sb == 0 || sb > sizeof(ws)) { printf("plov_sort_workspace(2, 8) = %zu\n", sb); ++failures; }
  EXPECT_ZERO(plov_sort_workspace(0, 8));
  EXPECT_ZERO(plov_sort_workspace(2, 0));
  EXPECT_ZERO(plov_sort_workspace(-1, 8));
  EXPECT_ZERO(plov_sort_workspace(2, -8));
  EXPECT_ZERO(plov_sort_workspace(1 << 16, 1 << 15));          // S * n = 2^31
  EXPECT_ZERO(plov_sort_workspace(0x7fffffff, 0x7fffffff));
  EXPECT_REJECT(plov_sort_descending(nullptr, 2, 8, out, perm, ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 2, 8, nullptr, perm, ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 2, 8, out, nullptr, ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 2, 8, out, perm, nullptr, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 0, 8, out, perm, ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 2, 0, out, perm, ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, -2, 8, out, perm, ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 2, -8, out, perm, ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 1 << 16, 1 << 15, out, perm, ws, sizeof(ws), nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 0x7fffffff, 0x7fffffff, out, perm, ws, sizeof(ws), nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 2, 8, out, perm, ws, sb - 1, nullptr));          // workspace too small
  EXPECT_REJECT(plov_sort_descending(z, 2, 8, out, perm, ws, 0, nullptr));
  EXPECT_REJECT(plov_sort_descending(off(z, 2), 2, 8, out, perm, ws, sb, nullptr));      // alignment
  EXPECT_REJECT(plov_sort_descending(z, 2, 8, off(out, 1), perm, ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 2, 8, out, (int*)((char*)perm + 2), ws, sb, nullptr));
  EXPECT_REJECT(plov_sort_descending(z, 2, 8, out, perm, ws + 4, sb, nullptr));

  // ---- the loss: N = 2, K = 3, H = W = 2
  for (int per_image = 0; per_image < 2; ++per_image) {
    const size_t lb = plov_loss_workspace(2, 3, 2, 2, per_image);
    if (lb == 0 || lb > sizeof(ws)) { printf("plov_loss_workspace(2, 3, 2, 2, %d) = %zu\n", per_image, lb); ++failures; }
    EXPECT_ZERO(plov_loss_workspace(0, 3, 2, 2, per_image));
    EXPECT_ZERO(plov_loss_workspace(2, 1, 2, 2, per_image));
    EXPECT_ZERO(plov_loss_workspace(2, 0, 2, 2, per_image));
    EXPECT_ZERO(plov_loss_workspace(2, 33, 2, 2, per_image));
    EXPECT_ZERO(plov_loss_workspace(2, -3, 2, 2, per_image));
    EXPECT_ZERO(plov_loss_workspace(2, 3, 0, 2, per_image));
    EXPECT_ZERO(plov_loss_workspace(2, 3, 2, -2, per_image));
    EXPECT_ZERO(plov_loss_workspace(-2, 3, 2, 2, per_image));
    EXPECT_ZERO(plov_loss_workspace(1 << 10, 2, 1 << 10, 1 << 10, per_image));          // 2^31
    EXPECT_ZERO(plov_loss_workspace(0x7fffffff, 32, 0x7fffffff, 0x7fffffff, per_image));
    // null pointers (errors and perm may be null, the others not)
    EXPECT_REJECT(fwd(nullptr, t, 2, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, nullptr, 2, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, nullptr, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, nullptr, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, nullptr, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, err, perm, nullptr, lb, 1, per_image));
    // sizes
    EXPECT_REJECT(fwd(z, t, 0, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, -2, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 0, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, -1, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 1, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 0, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 33, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 1 << 10, 2, 1 << 10, 1 << 10, loss, w, sc, err, perm, ws, sizeof(ws), 1, per_image));
    EXPECT_REJECT(fwd(z, t, 0x7fffffff, 32, 0x7fffffff, 0x7fffffff, loss, w, sc, err, perm, ws, sizeof(ws), 1, per_image));
    // workspace too small, flags that are not flags, alignment
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, err, perm, ws, lb - 1, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, err, perm, ws, 0, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 2, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image, 7));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image + 2));
    EXPECT_REJECT(fwd(off(z, 1), t, 2, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, (const long long*)((const char*)t + 4), 2, 3, 2, 2, loss, w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, off(loss, 2), w, sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, off(w, 3), sc, err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, off(sc, 1), err, perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, off(err, 2), perm, ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, err, (int*)((char*)perm + 1), ws, lb, 1, per_image));
    EXPECT_REJECT(fwd(z, t, 2, 3, 2, 2, loss, w, sc, err, perm, ws + 4, lb, 1, per_image));

    EXPECT_REJECT(bwd(nullptr, t, 2, 3, 2, 2, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, nullptr, 2, 3, 2, 2, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, nullptr, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, w, nullptr, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, w, sc, nullptr, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, w, sc, up, nullptr, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 0, 3, 2, 2, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, -2, 2, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 0, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 1, 2, 2, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 33, 2, 2, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 1 << 10, 2, 1 << 10, 1 << 10, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 0x7fffffff, 32, 0x7fffffff, 0x7fffffff, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, w, sc, up, out, -1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, w, sc, up, out, 1, per_image + 2));
    EXPECT_REJECT(bwd(off(z, 2), t, 2, 3, 2, 2, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, (const long long*)((const char*)t + 2), 2, 3, 2, 2, w, sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, off(w, 1), sc, up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, w, off(sc, 2), up, out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, w, sc, off(up, 3), out, 1, per_image));
    EXPECT_REJECT(bwd(z, t, 2, 3, 2, 2, w, sc, up, off(out, 1), 1, per_image));
  }

  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("asan_lov_args: all argument checks rejected their input, no sanitizer report\n");
  return 0;
}
