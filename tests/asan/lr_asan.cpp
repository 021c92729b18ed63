// Host-side AddressSanitizer run of the left-right check's two entries
// (lea_disparity_regression_right, lea_disparity_lr_check), built and run by `make asan`
// after the other two drivers, the same way: every csrc unit with ASan on its host side,
// nothing launched.  Each refused call must return the documented code, leave a
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

int main() {
  if (lea_abi_version() != 14) {
    std::printf("FAIL abi version %d\n", lea_abi_version());
    ++g_fail;
  }
  // B = 1, D3 = 4, H3 = 2, W3 = 2: cost 16 floats, disp_right 36 floats; host memory, the
  // checks never dereference it
  constexpr int kOut = 36;
  static float cost[16], buf[4 * kOut];
  static uint8_t bytes[2 * kOut];
  for (float& v : buf) v = -7.f;
  for (uint8_t& v : bytes) v = 9;
  {
    const char* who = "lea_disparity_regression_right";
    auto call = [&](const void* c, float* o, int B, int D3, int H3, int W3, int md, int dt) {
      return lea_disparity_regression_right(c, o, B, D3, H3, W3, md, dt, nullptr);
    };
    expect_err(who, "null cost", call(nullptr, buf, 1, 4, 2, 2, 12, LEA_F32), LEA_E_INVALID);
    expect_err(who, "null output", call(cost, nullptr, 1, 4, 2, 2, 12, LEA_F32), LEA_E_INVALID);
    expect_err(who, "B = 0", call(cost, buf, 0, 4, 2, 2, 12, LEA_F32), LEA_E_INVALID);
    expect_err(who, "D3 < 0", call(cost, buf, 1, -4, 2, 2, 12, LEA_F32), LEA_E_INVALID);
    expect_err(who, "H3 = 0", call(cost, buf, 1, 4, 0, 2, 12, LEA_F32), LEA_E_INVALID);
    expect_err(who, "W3 = 0", call(cost, buf, 1, 4, 2, 0, 12, LEA_F32), LEA_E_INVALID);
    expect_err(who, "maxdisp = 0", call(cost, buf, 1, 4, 2, 2, 0, LEA_F32), LEA_E_INVALID);
    expect_err(who, "dtype", call(cost, buf, 1, 4, 2, 2, 12, 7), LEA_E_UNSUPPORTED);
    expect_err(who, "maxdisp != 3 D3", call(cost, buf, 1, 4, 2, 2, 13, LEA_F32), LEA_E_UNSUPPORTED);
    expect_err(who, "maxdisp 2 D3", call(cost, buf, 1, 4, 2, 2, 8, LEA_BF16), LEA_E_UNSUPPORTED);
    expect_err(who, "in place", call(buf, buf, 1, 4, 2, 2, 12, LEA_F32), LEA_E_INVALID);
    expect_err(who, "output starts in the cost's last element", call(buf, buf + 15, 1, 4, 2, 2, 12, LEA_F32),
               LEA_E_INVALID);
    expect_err(who, "cost starts in the output's last element", call(buf + kOut - 1, buf, 1, 4, 2, 2, 12, LEA_F32),
               LEA_E_INVALID);
  }
  {
    // B = 1, H = 6, W = 6: 36 floats each, 36 bytes of state
    const char* who = "lea_disparity_lr_check";
    float *dl = buf, *dr = buf + kOut, *fi = buf + 2 * kOut, *spare = buf + 3 * kOut;
    auto call = [&](const float* l, const float* r, uint8_t* s, float* f, int B, int H, int W, float thr) {
      return lea_disparity_lr_check(l, r, s, f, B, H, W, thr, nullptr);
    };
    expect_err(who, "null disp_left", call(nullptr, dr, bytes, fi, 1, 6, 6, 1.f), LEA_E_INVALID);
    expect_err(who, "null disp_right", call(dl, nullptr, bytes, fi, 1, 6, 6, 1.f), LEA_E_INVALID);
    expect_err(who, "both outputs null", call(dl, dr, nullptr, nullptr, 1, 6, 6, 1.f), LEA_E_INVALID);
    expect_err(who, "B = 0", call(dl, dr, bytes, fi, 0, 6, 6, 1.f), LEA_E_INVALID);
    expect_err(who, "H < 0", call(dl, dr, bytes, fi, 1, -6, 6, 1.f), LEA_E_INVALID);
    expect_err(who, "W = 0", call(dl, dr, bytes, fi, 1, 6, 0, 1.f), LEA_E_INVALID);
    expect_err(who, "threshold 0", call(dl, dr, bytes, fi, 1, 6, 6, 0.f), LEA_E_INVALID);
    expect_err(who, "threshold < 0", call(dl, dr, bytes, fi, 1, 6, 6, -1.f), LEA_E_INVALID);
    expect_err(who, "threshold NaN", call(dl, dr, bytes, fi, 1, 6, 6, std::nanf("")), LEA_E_INVALID);
    expect_err(who, "threshold inf", call(dl, dr, bytes, fi, 1, 6, 6, std::numeric_limits<float>::infinity()),
               LEA_E_INVALID);
    expect_err(who, "filled = disp_left", call(dl, dr, bytes, dl, 1, 6, 6, 1.f), LEA_E_INVALID);
    expect_err(who, "filled inside disp_right", call(dl, dr, bytes, dr + kOut - 1, 1, 6, 6, 1.f), LEA_E_INVALID);
    expect_err(who, "state inside disp_left", call(dl, dr, (uint8_t*)(dl + kOut) - 1, fi, 1, 6, 6, 1.f),
               LEA_E_INVALID);
    expect_err(who, "state inside disp_right", call(dl, dr, (uint8_t*)dr, nullptr, 1, 6, 6, 1.f), LEA_E_INVALID);
    expect_err(who, "state inside filled", call(dl, dr, (uint8_t*)spare + 4 * kOut - 1, spare, 1, 6, 6, 1.f),
               LEA_E_INVALID);
    expect_err(who, "filled starts in the state's last byte", call(dl, dr, (uint8_t*)fi - kOut + 1, fi, 1, 6, 6, 1.f),
               LEA_E_INVALID);
  }
  for (float v : buf)
    if (v != -7.f) {
      std::printf("FAIL a refused call wrote to a buffer\n");
      ++g_fail;
      break;
    }
  for (uint8_t v : bytes)
    if (v != 9) {
      std::printf("FAIL a refused call wrote to the state bytes\n");
      ++g_fail;
      break;
    }
  std::printf("%s lr: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
