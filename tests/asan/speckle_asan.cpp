// Host-side AddressSanitizer run of the speckle filter's two entries
// (lea_disparity_speckle_workspace_bytes, lea_disparity_speckle_f32), built and run by
// `make asan` after the other drivers, the same way: every csrc unit with ASan on its host
// side, nothing launched.  Each refused call must return LEA_E_INVALID, leave a
// lea_last_error() that names the entry, and touch none of its buffers.
// Exit 0 = every check passed and ASan saw no error.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "leastereo_hip.h"

static int g_fail = 0;

static void expect_err(const char* entry, const char* what, int rc, int want) {
  const char* e = lea_last_error();
  if (rc != want || e == nullptr || std::strstr(e, entry) == nullptr) {
    std::printf("FAIL %s %s: rc=%d (want %d) err='%s'\n", entry, what, rc, want, e ? e : "(null)");
    ++g_fail;
  }
}

static void expect_bytes(const char* what, size_t got, size_t want) {
  if (got != want) {
    std::printf("FAIL workspace bytes %s: %zu (want %zu)\n", what, got, want);
    ++g_fail;
  }
}

int main() {
  if (lea_abi_version() != 14) {
    std::printf("FAIL abi version %d\n", lea_abi_version());
    ++g_fail;
  }
  expect_bytes("2x6x7", lea_disparity_speckle_workspace_bytes(2, 6, 7), 8 * 84);
  expect_bytes("1x1x1", lea_disparity_speckle_workspace_bytes(1, 1, 1), 8);
  expect_bytes("1x2048x2048", lea_disparity_speckle_workspace_bytes(1, 2048, 2048), (size_t)8 << 22);
  expect_bytes("3x40000x50000", lea_disparity_speckle_workspace_bytes(3, 40000, 50000), (size_t)48000000000ull);
  expect_bytes("B = 0", lea_disparity_speckle_workspace_bytes(0, 6, 7), 0);
  expect_bytes("H < 0", lea_disparity_speckle_workspace_bytes(2, -6, 7), 0);
  expect_bytes("W = 0", lea_disparity_speckle_workspace_bytes(2, 6, 0), 0);

  // B = 2, H = 6, W = 7: a map is 84 elements, the workspace 168 ints; host memory, the checks
  // never dereference it
  constexpr int kMap = 84, kWs = 168;
  static float disp[kMap], filt[kMap];
  static int32_t ws[kWs + kMap], lab[kMap], siz[kMap];
  static uint8_t ex[kMap], st[kMap + 4];
  auto reset = [&]() {
    for (int k = 0; k < kMap; ++k) disp[k] = filt[k] = -7.f, lab[k] = siz[k] = -7, ex[k] = 9;
    for (int k = 0; k < kWs + kMap; ++k) ws[k] = -7;
    for (uint8_t& v : st) v = 9;
  };
  reset();
  const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();
  const char* who = "lea_disparity_speckle_f32";
  auto call = [&](const float* d, const uint8_t* e, int B, int H, int W, float md, int ms, float fill, void* w,
                  int32_t* l, int32_t* s, uint8_t* t, float* f) {
    return lea_disparity_speckle_f32(d, e, B, H, W, md, ms, fill, w, l, s, t, f, nullptr);
  };
  expect_err(who, "null disp", call(nullptr, ex, 2, 6, 7, 1.f, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "null workspace", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, nullptr, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "every output null", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, nullptr, nullptr, nullptr, nullptr),
             LEA_E_INVALID);
  expect_err(who, "B = 0", call(disp, ex, 0, 6, 7, 1.f, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "B < 0", call(disp, ex, -2, 6, 7, 1.f, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "H < 0", call(disp, ex, 2, -6, 7, 1.f, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "W = 0", call(disp, ex, 2, 6, 0, 1.f, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "B too large", call(disp, ex, 65536, 6, 7, 1.f, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "H*W = 2^31", call(disp, ex, 1, 1 << 16, 1 << 15, 1.f, 20, 0.f, ws, lab, siz, st, filt),
             LEA_E_INVALID);
  expect_err(who, "H*W = 2^40", call(disp, ex, 1, 1 << 20, 1 << 20, 1.f, 20, 0.f, ws, lab, siz, st, filt),
             LEA_E_INVALID);
  expect_err(who, "H too large", call(disp, ex, 1, 1048561, 1, 1.f, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "max_diff < 0", call(disp, ex, 2, 6, 7, -1.f, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "max_diff NaN", call(disp, ex, 2, 6, 7, nan, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "max_diff inf", call(disp, ex, 2, 6, 7, inf, 20, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "max_size < 0", call(disp, ex, 2, 6, 7, 1.f, -1, 0.f, ws, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "misaligned workspace", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, (char*)ws + 2, lab, siz, st, filt),
             LEA_E_INVALID);
  expect_err(who, "filtered = disp", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, lab, siz, st, disp), LEA_E_INVALID);
  expect_err(who, "labels = disp", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, (int32_t*)disp, siz, st, filt),
             LEA_E_INVALID);
  expect_err(who, "state = exclude", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, lab, siz, ex, filt), LEA_E_INVALID);
  expect_err(who, "state starts in exclude's last byte",
             call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, lab, siz, ex + kMap - 1, filt), LEA_E_INVALID);
  expect_err(who, "size in the workspace's last element",
             call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, lab, ws + kWs - 1, st, filt), LEA_E_INVALID);
  expect_err(who, "labels = size", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, lab, lab, st, filt), LEA_E_INVALID);
  expect_err(who, "filtered = size", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, lab, siz, st, (float*)siz),
             LEA_E_INVALID);
  expect_err(who, "state in filtered's last byte",
             call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, ws, lab, siz, (uint8_t*)filt + 4 * kMap - 1, filt), LEA_E_INVALID);
  expect_err(who, "workspace = disp", call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, disp, lab, siz, st, filt), LEA_E_INVALID);
  expect_err(who, "workspace ends in exclude",
             call(disp, ex, 2, 6, 7, 1.f, 20, 0.f, (void*)(((uintptr_t)ex & ~(uintptr_t)3) - 4 * (kWs - 1)), lab, siz, st,
                  filt),
             LEA_E_INVALID);
  // the optional ones may be null: the next check in line fires
  expect_err(who, "null exclude, labels, size, filtered, then max_size",
             call(disp, nullptr, 2, 6, 7, 1.f, -5, nan, ws, nullptr, nullptr, st, nullptr), LEA_E_INVALID);

  bool wrote = false;
  for (int k = 0; k < kMap; ++k)
    wrote |= disp[k] != -7.f || filt[k] != -7.f || lab[k] != -7 || siz[k] != -7 || ex[k] != 9;
  for (int k = 0; k < kWs + kMap; ++k) wrote |= ws[k] != -7;
  for (uint8_t v : st) wrote |= v != 9;
  if (wrote) {
    std::printf("FAIL a refused call wrote to a buffer\n");
    ++g_fail;
  }
  std::printf("%s speckle: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
