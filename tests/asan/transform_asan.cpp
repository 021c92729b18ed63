// Host-side AddressSanitizer run of the training transform's two entries
// (lea_train_transform_workspace_bytes, lea_train_transform_u8), built and run by `make asan`
// after the other drivers, the same way: every csrc unit with ASan on its host side, nothing
// launched.  Each refused call must return LEA_E_INVALID, leave a lea_last_error() that names
// the entry, and touch none of its buffers.
// Exit 0 = every check passed and ASan saw no error.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "leastereo_hip.h"

static int g_fail = 0;

static void expect_err(const char* entry, const char* what, int rc, int want) {
  const char* e = lea_last_error();
  if (rc != want || e == nullptr || std::strstr(e, entry) == nullptr) {
    std::printf("FAIL %s %s: rc=%d (want %d) err='%s'\n", entry, what, rc, want, e ? e : "(null)");
    ++g_fail;
  }
}

int main() {
  if (lea_abi_version() != 14) {
    std::printf("FAIL abi version %d\n", lea_abi_version());
    ++g_fail;
  }
  if (lea_train_transform_workspace_bytes(2) != 2 * 2 * 3 * 2 * sizeof(unsigned long long) ||
      lea_train_transform_workspace_bytes(2) != lea_standardize_workspace_bytes(2) ||
      lea_train_transform_workspace_bytes(0) != 0 || lea_train_transform_workspace_bytes(-3) != 0) {
    std::printf("FAIL lea_train_transform_workspace_bytes\n");
    ++g_fail;
  }
  // B = 2, H = 6, W = 7, RGB -> crop 4 x 8; host memory, the checks never dereference it
  constexpr int kPix = 2 * 6 * 7, kCrop = 2 * 4 * 8;
  alignas(16) static unsigned char img[2][kPix * 3];
  alignas(16) static float disp[2][kPix];
  alignas(16) static float out[3][3 * kCrop];
  alignas(16) static int params[2 * 5 + 2];
  alignas(16) static unsigned long long ws[2 * 2 * 3 * 2];
  std::memset(img, 0x5a, sizeof img);
  for (auto& d : disp)
    for (float& v : d) v = -7.f;
  for (auto& o : out)
    for (float& v : o) v = -7.f;
  for (int& v : params) v = -7;
  for (auto& v : ws) v = 7;
  int* nv = params + 10;
  const char* who = "lea_train_transform_u8";
  auto call = [&](const void* l, const void* r, int B, int H, int W, int ps, const float* dl, const float* dr,
                  const int* p, float* ol, float* orr, float* ot, int ch, int cw, float md, int* n, void* w) {
    return lea_train_transform_u8(l, r, B, H, W, ps, dl, dr, p, ol, orr, ot, ch, cw, md, n, w, nullptr);
  };
  const void *L = img[0], *R = img[1];
  const float *DL = disp[0], *DR = disp[1];
  float *OL = out[0], *OR = out[1], *OT = out[2];
  expect_err(who, "null left", call(nullptr, R, 2, 6, 7, 3, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "null right", call(L, nullptr, 2, 6, 7, 3, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "null disp_left", call(L, R, 2, 6, 7, 3, nullptr, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws),
             LEA_E_INVALID);
  expect_err(who, "null params", call(L, R, 2, 6, 7, 3, DL, DR, nullptr, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "null out_left", call(L, R, 2, 6, 7, 3, DL, DR, params, nullptr, OR, OT, 4, 8, 48.f, nv, ws),
             LEA_E_INVALID);
  expect_err(who, "null out_right", call(L, R, 2, 6, 7, 3, DL, DR, params, OL, nullptr, OT, 4, 8, 48.f, nv, ws),
             LEA_E_INVALID);
  expect_err(who, "null out_target", call(L, R, 2, 6, 7, 3, DL, DR, params, OL, OR, nullptr, 4, 8, 48.f, nv, ws),
             LEA_E_INVALID);
  expect_err(who, "null workspace", call(L, R, 2, 6, 7, 3, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, nullptr),
             LEA_E_INVALID);
  expect_err(who, "B = 0", call(L, R, 0, 6, 7, 3, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "H < 0", call(L, R, 2, -6, 7, 3, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "W = 0", call(L, R, 2, 6, 0, 3, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "crop_h = 0", call(L, R, 2, 6, 7, 3, DL, DR, params, OL, OR, OT, 0, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "crop_w < 0", call(L, R, 2, 6, 7, 3, DL, DR, params, OL, OR, OT, 4, -8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "pix_stride 2", call(L, R, 2, 6, 7, 2, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "pix_stride 5", call(L, R, 2, 6, 7, 5, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "image of 2^31 pixels",
             call(L, R, 2, 1 << 16, 1 << 15, 3, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "crop of 2^31 pixels",
             call(L, R, 2, 6, 7, 3, DL, DR, params, OL, OR, OT, 1 << 16, 1 << 15, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "maxdisp NaN", call(L, R, 2, 6, 7, 3, DL, DR, params, OL, OR, OT, 4, 8, std::nanf(""), nv, ws),
             LEA_E_INVALID);
  expect_err(who, "misaligned target, crop_w % 4 == 0",
             call(L, R, 2, 6, 7, 3, DL, DR, params, OL, OR, OT + 1, 4, 8, 48.f, nv, ws), LEA_E_INVALID);
  expect_err(who, "misaligned params",
             call(L, R, 2, 6, 7, 3, DL, DR, (const int*)((const char*)params + 2), OL, OR, OT, 4, 8, 48.f, nv, ws),
             LEA_E_INVALID);
  expect_err(who, "misaligned workspace",
             call(L, R, 2, 6, 7, 3, DL, DR, params, OL, OR, OT, 4, 8, 48.f, nv, (char*)ws + 4), LEA_E_INVALID);
  // the optional pointers are not what a refusal is about: still the shape
  expect_err(who, "B = 0 without disp_right and n_valid",
             call(L, R, 0, 6, 7, 3, DL, nullptr, params, OL, OR, OT, 4, 8, 48.f, nullptr, ws), LEA_E_INVALID);
  bool wrote = false;
  for (auto& o : out)
    for (float v : o) wrote = wrote || v != -7.f;
  if (wrote) {
    std::printf("FAIL a refused call wrote to an output\n");
    ++g_fail;
  }
  for (int v : params)
    if (v != -7) {
      std::printf("FAIL a refused call wrote to the params or n_valid\n");
      ++g_fail;
      break;
    }
  for (auto v : ws)
    if (v != 7) {
      std::printf("FAIL a refused call wrote to the workspace\n");
      ++g_fail;
      break;
    }
  std::printf("%s transform: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
