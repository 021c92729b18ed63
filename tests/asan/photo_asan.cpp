// Host-side AddressSanitizer run of the photometric-consistency entries
// (lea_photometric_workspace_bytes, lea_photometric_f32, lea_photometric_grad_f32), built
// and run by `make asan` after the other five drivers, the same way: every csrc unit with
// ASan on its host side, nothing launched.  Host argument checks and the workspace query
// only.  Each refused call must return LEA_E_INVALID, leave a lea_last_error() that names
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
  // B = 2, C = 3, H = 6, W = 7: an image is 252 floats, a map 84; host memory, the checks
  // never dereference it
  constexpr int kHW = 42, kMap = 2 * kHW, kCHW = 3 * kHW, kImg = 2 * kCHW;
  static float img[3 * kImg];   // left, right, warped
  static float map[3 * kMap];   // disp, err, ddisp
  static uint8_t excl[kMap];
  static double sums[4 + 8];    // the sums, then a workspace of two workgroups' partials
  static float scales[2] = {0.15f, 0.85f};
  for (float& v : img) v = -7.f;
  for (float& v : map) v = -7.f;
  for (double& v : sums) v = -7.0;
  std::memset(excl, 3, sizeof excl);
  float *left = img, *right = img + kImg, *warped = img + 2 * kImg;
  float *disp = map, *err = map + kMap, *ddisp = map + 2 * kMap;
  double* ws = sums + 4;
  if (lea_photometric_workspace_bytes(2, 6, 7) != 2 * 4 * sizeof(double) ||
      lea_photometric_workspace_bytes(2, 17, 65) != 8 * 4 * sizeof(double) ||
      lea_photometric_workspace_bytes(2, 0, 7) != 0 || lea_photometric_workspace_bytes(-1, 6, 7) != 0) {
    std::printf("FAIL lea_photometric_workspace_bytes\n");
    ++g_fail;
  }
  {
    const char* who = "lea_photometric_f32";
    struct A {
      const float *l, *r, *d;
      const uint8_t* e;
      int64_t lbs, rbs, dbs, ebs;
      int B, C, H, W;
      float alpha, c1, c2;
      double* su;
      void* w;
      float *wp, *er;
    };
    const A ok{left, right, disp, excl, kCHW, kCHW, kHW, kHW, 2, 3, 6, 7, 0.85f, 1e-4f, 9e-4f, sums, ws, warped, err};
    auto call = [&](const A& a) {
      return lea_photometric_f32(a.l, a.lbs, a.r, a.rbs, a.d, a.dbs, a.e, a.ebs, a.B, a.C, a.H, a.W, a.alpha, a.c1,
                                 a.c2, a.su, a.w, a.wp, a.er, nullptr);
    };
    A a = ok;
    a.l = nullptr; expect_err(who, "null left", call(a), LEA_E_INVALID); a = ok;
    a.r = nullptr; expect_err(who, "null right", call(a), LEA_E_INVALID); a = ok;
    a.d = nullptr; expect_err(who, "null disp", call(a), LEA_E_INVALID); a = ok;
    a.su = nullptr; expect_err(who, "null sums", call(a), LEA_E_INVALID); a = ok;
    a.w = nullptr; expect_err(who, "null workspace", call(a), LEA_E_INVALID); a = ok;
    a.B = 0; expect_err(who, "B = 0", call(a), LEA_E_INVALID); a = ok;
    a.C = 0; expect_err(who, "C = 0", call(a), LEA_E_INVALID); a = ok;
    a.C = 5; expect_err(who, "C = 5", call(a), LEA_E_INVALID); a = ok;
    a.H = 2; expect_err(who, "H = 2", call(a), LEA_E_INVALID); a = ok;
    a.W = 2; expect_err(who, "W = 2", call(a), LEA_E_INVALID); a = ok;
    a.lbs = kCHW - 1; expect_err(who, "left stride below C*H*W", call(a), LEA_E_INVALID); a = ok;
    a.rbs = kHW; expect_err(who, "right stride below C*H*W", call(a), LEA_E_INVALID); a = ok;
    a.dbs = kHW - 1; expect_err(who, "disp stride below H*W", call(a), LEA_E_INVALID); a = ok;
    a.ebs = 0; expect_err(who, "exclude stride below H*W", call(a), LEA_E_INVALID); a = ok;
    a.alpha = -0.5f; expect_err(who, "alpha < 0", call(a), LEA_E_INVALID); a = ok;
    a.alpha = 1.5f; expect_err(who, "alpha > 1", call(a), LEA_E_INVALID); a = ok;
    a.alpha = std::nanf(""); expect_err(who, "alpha NaN", call(a), LEA_E_INVALID); a = ok;
    a.c1 = 0.f; expect_err(who, "c1 = 0", call(a), LEA_E_INVALID); a = ok;
    a.c2 = -9e-4f; expect_err(who, "c2 < 0", call(a), LEA_E_INVALID); a = ok;
    a.su = (double*)((char*)sums + 4); expect_err(who, "misaligned sums", call(a), LEA_E_INVALID); a = ok;
    a.w = (char*)ws + 4; expect_err(who, "misaligned workspace", call(a), LEA_E_INVALID); a = ok;
    a.w = sums + 3; expect_err(who, "workspace inside sums", call(a), LEA_E_INVALID); a = ok;
    a.wp = left; expect_err(who, "warped = left", call(a), LEA_E_INVALID); a = ok;
    a.wp = right + kImg - 1; expect_err(who, "warped starts in right's last element", call(a), LEA_E_INVALID); a = ok;
    a.er = disp; expect_err(who, "err = disp", call(a), LEA_E_INVALID); a = ok;
    a.er = (float*)(void*)excl; expect_err(who, "err over exclude", call(a), LEA_E_INVALID); a = ok;
    a.er = warped + kImg - 1; expect_err(who, "err starts in warped's last element", call(a), LEA_E_INVALID); a = ok;
    a.su = (double*)(void*)left; expect_err(who, "sums over left", call(a), LEA_E_INVALID); a = ok;
    a.w = disp; expect_err(who, "workspace over disp", call(a), LEA_E_INVALID); a = ok;
  }
  {
    const char* who = "lea_photometric_grad_f32";
    struct A {
      const float *l, *r, *d;
      const uint8_t* e;
      int64_t lbs, rbs, dbs, ebs;
      int B, C, H, W;
      float c1, c2;
      const double* su;
      const float* sc;
      float* g;
      int64_t gbs;
    };
    const A ok{left, right, disp, excl, kCHW, kCHW, kHW, kHW, 2, 3, 6, 7, 1e-4f, 9e-4f, sums, scales, ddisp, kHW};
    auto call = [&](const A& a) {
      return lea_photometric_grad_f32(a.l, a.lbs, a.r, a.rbs, a.d, a.dbs, a.e, a.ebs, a.B, a.C, a.H, a.W, a.c1, a.c2,
                                      a.su, a.sc, a.g, a.gbs, nullptr);
    };
    A a = ok;
    a.l = nullptr; expect_err(who, "null left", call(a), LEA_E_INVALID); a = ok;
    a.r = nullptr; expect_err(who, "null right", call(a), LEA_E_INVALID); a = ok;
    a.d = nullptr; expect_err(who, "null disp", call(a), LEA_E_INVALID); a = ok;
    a.su = nullptr; expect_err(who, "null sums", call(a), LEA_E_INVALID); a = ok;
    a.sc = nullptr; expect_err(who, "null scales", call(a), LEA_E_INVALID); a = ok;
    a.g = nullptr; expect_err(who, "null ddisp", call(a), LEA_E_INVALID); a = ok;
    a.C = 5; expect_err(who, "C = 5", call(a), LEA_E_INVALID); a = ok;
    a.H = 2; expect_err(who, "H = 2", call(a), LEA_E_INVALID); a = ok;
    a.W = 1; expect_err(who, "W = 1", call(a), LEA_E_INVALID); a = ok;
    a.lbs = 0; expect_err(who, "left stride 0", call(a), LEA_E_INVALID); a = ok;
    a.gbs = kHW - 1; expect_err(who, "ddisp stride below H*W", call(a), LEA_E_INVALID); a = ok;
    a.c1 = std::nanf(""); expect_err(who, "c1 NaN", call(a), LEA_E_INVALID); a = ok;
    a.c2 = 0.f; expect_err(who, "c2 = 0", call(a), LEA_E_INVALID); a = ok;
    a.su = (const double*)((const char*)sums + 4); expect_err(who, "misaligned sums", call(a), LEA_E_INVALID); a = ok;
    a.g = disp; expect_err(who, "ddisp = disp", call(a), LEA_E_INVALID); a = ok;
    a.g = left + kImg - 1; expect_err(who, "ddisp starts in left's last element", call(a), LEA_E_INVALID); a = ok;
    a.r = ddisp + kMap - 1; expect_err(who, "right starts in ddisp's last element", call(a), LEA_E_INVALID); a = ok;
    a.g = (float*)(void*)excl; expect_err(who, "ddisp over exclude", call(a), LEA_E_INVALID); a = ok;
    a.g = scales + 1; expect_err(who, "ddisp over the scales", call(a), LEA_E_INVALID); a = ok;
    a.g = (float*)(void*)(sums + 3); expect_err(who, "ddisp over the sums", call(a), LEA_E_INVALID); a = ok;
  }
  for (float v : img)
    if (v != -7.f) {
      std::printf("FAIL a refused call wrote to an image\n");
      ++g_fail;
      break;
    }
  for (float v : map)
    if (v != -7.f) {
      std::printf("FAIL a refused call wrote to a map\n");
      ++g_fail;
      break;
    }
  for (double v : sums)
    if (v != -7.0) {
      std::printf("FAIL a refused call wrote to the sums or the workspace\n");
      ++g_fail;
      break;
    }
  for (uint8_t v : excl)
    if (v != 3) {
      std::printf("FAIL a refused call wrote to exclude\n");
      ++g_fail;
      break;
    }
  if (scales[0] != 0.15f || scales[1] != 0.85f) {
    std::printf("FAIL a refused call wrote to the scales\n");
    ++g_fail;
  }
  std::printf("%s photo: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
