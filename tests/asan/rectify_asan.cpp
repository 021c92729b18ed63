// Host-side AddressSanitizer run of the rectification's entries (lea_rectify_pair_u8,
// lea_rectify_set_tile), built and run by `make asan` after the other drivers, the same way:
// every csrc unit with ASan on its host side, nothing launched.  Each refused call must return
// LEA_E_INVALID, leave a lea_last_error() that names the entry, and touch none of its buffers.
// Exit 0 = every check passed and ASan saw no error.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "leastereo_hip.h"
#include "leastereo_hip_tuning.h"

static int g_fail = 0;

static void expect_err(const char* entry, const char* what, int rc, int want) {
  const char* e = lea_last_error();
  if (rc != want || e == nullptr || std::strstr(e, entry) == nullptr) {
    std::printf("FAIL %s %s: rc=%d (want %d) err='%s'\n", entry, what, rc, want, e ? e : "(null)");
    ++g_fail;
  }
}

// B = 2, raw 5 x 6, rectified 4 x 7, pixel stride up to 4
constexpr int kB = 2, kH = 5, kW = 6, kHo = 4, kWo = 7;
constexpr int kIn = kB * kH * kW * 4, kOut = kB * kHo * kWo * 4, kVal = kB * 2 * kHo * kWo, kMap = kB * 4 * kHo * kWo;
static uint8_t L[kIn], R[kIn], OL[kOut], OR_[kOut], V[kVal];
static float C[kB * 48], MI[kMap], MO[kMap];

struct Args {
  const void* l = L;
  const void* r = R;
  int ps = 3, B = kB, H = kH, W = kW;
  const float* c = C;
  int Bc = kB;
  const float* mi = nullptr;
  int Bm = 0, Ho = kHo, Wo = kWo, fill = 0;
  void* ol = OL;
  void* orr = OR_;
  uint8_t* v = V;
  float* mo = MO;
};

static int call(const Args& a) {
  return lea_rectify_pair_u8(a.l, a.r, a.ps, a.B, a.H, a.W, a.c, a.Bc, a.mi, a.Bm, a.Ho, a.Wo, a.fill, a.ol, a.orr,
                             a.v, a.mo, nullptr);
}

template <class F>
static void refused(const char* what, F change) {
  Args a;
  change(a);
  expect_err("lea_rectify_pair_u8", what, call(a), LEA_E_INVALID);
}

int main() {
  if (lea_abi_version() != 14) {
    std::printf("FAIL abi version %d\n", lea_abi_version());
    ++g_fail;
  }
  auto reset = [&]() {
    std::memset(L, 9, sizeof L), std::memset(R, 9, sizeof R), std::memset(OL, 9, sizeof OL);
    std::memset(OR_, 9, sizeof OR_), std::memset(V, 9, sizeof V);
    for (float& x : C) x = -7.f;
    for (float& x : MI) x = -7.f;
    for (float& x : MO) x = -7.f;
  };
  reset();
  auto with_maps = [](Args& a) { a.c = nullptr, a.Bc = 0, a.mi = MI, a.Bm = kB; };

  refused("null left", [](Args& a) { a.l = nullptr; });
  refused("null right", [](Args& a) { a.r = nullptr; });
  refused("null out_left", [](Args& a) { a.ol = nullptr; });
  refused("null out_right", [](Args& a) { a.orr = nullptr; });
  refused("pix_stride 2", [](Args& a) { a.ps = 2; });
  refused("pix_stride 5", [](Args& a) { a.ps = 5; });
  refused("pix_stride 0", [](Args& a) { a.ps = 0; });
  refused("B = 0", [](Args& a) { a.B = 0; });
  refused("B < 0", [](Args& a) { a.B = -2; });
  refused("H = 0", [](Args& a) { a.H = 0; });
  refused("W < 0", [](Args& a) { a.W = -6; });
  refused("Ho = 0", [](Args& a) { a.Ho = 0; });
  refused("Wo < 0", [](Args& a) { a.Wo = -1; });
  refused("B too large", [](Args& a) { a.B = 32768, a.Bc = 1; });
  refused("H too large", [](Args& a) { a.H = 65536; });
  refused("Wo too large", [](Args& a) { a.Wo = 1 << 20; });
  refused("calib and maps_in", [](Args& a) { a.mi = MI, a.Bm = kB; });
  refused("neither calib nor maps_in", [](Args& a) { a.c = nullptr; });
  refused("Bc = 0", [](Args& a) { a.Bc = 0; });
  refused("Bc = 3", [](Args& a) { a.Bc = 3; });
  refused("Bc = -1", [](Args& a) { a.Bc = -1; });
  refused("Bm = 0", [&](Args& a) { with_maps(a), a.Bm = 0; });
  refused("Bm = 3", [&](Args& a) { with_maps(a), a.Bm = 3; });
  refused("fill 256", [](Args& a) { a.fill = 256; });
  refused("fill -1", [](Args& a) { a.fill = -1; });
  refused("misaligned calib", [](Args& a) { a.c = (const float*)((const char*)C + 2); });
  refused("misaligned maps_in", [&](Args& a) { with_maps(a), a.mi = (const float*)((const char*)MI + 1); });
  refused("misaligned maps_out", [](Args& a) { a.mo = (float*)((char*)MO + 2); });
  // an output on an input
  refused("out_left = left", [](Args& a) { a.ol = L; });
  refused("out_right = left", [](Args& a) { a.orr = L; });
  refused("out_left in right's last byte (stride 4)", [](Args& a) { a.ps = 4, a.ol = R + kIn - 1; });
  refused("valid = right", [](Args& a) { a.v = R; });
  refused("maps_out = calib", [](Args& a) { a.mo = C; });
  refused("maps_out in calib's last float", [](Args& a) { a.mo = C + kB * 48 - 1; });
  refused("out_left = calib", [](Args& a) { a.ol = C; });
  refused("maps_out = maps_in", [&](Args& a) { with_maps(a), a.mo = MI; });
  refused("valid in maps_in's last byte", [&](Args& a) { with_maps(a), a.v = (uint8_t*)MI + 4 * kMap - 1; });
  // an output on another output
  refused("out_right = out_left", [](Args& a) { a.orr = OL; });
  refused("out_right in out_left's last byte (stride 4)", [](Args& a) { a.ps = 4, a.orr = OL + kOut - 1; });
  refused("valid = out_left", [](Args& a) { a.v = OL; });
  refused("maps_out on valid", [](Args& a) { a.mo = (float*)(((uintptr_t)V + 3) & ~(uintptr_t)3); });
  // the optional ones may be null, and with one calibration for all only its 48 floats are
  // calib: an output behind them is no overlap, and the next check in line fires
  refused("null valid and maps_out, then the overlap", [](Args& a) { a.v = nullptr, a.mo = nullptr, a.orr = OL; });
  refused("Bc = 1, maps_out behind the block, then the overlap", [](Args& a) {
    a.Bc = 1, a.mo = C + 48, a.orr = OL;
  });

  expect_err("lea_rectify_set_tile", "mode 2", lea_rectify_set_tile(2), LEA_E_INVALID);
  expect_err("lea_rectify_set_tile", "mode -1", lea_rectify_set_tile(-1), LEA_E_INVALID);
  if (lea_rectify_set_tile(1) != LEA_OK || lea_rectify_set_tile(0) != LEA_OK) {
    std::printf("FAIL lea_rectify_set_tile refuses 0 or 1\n");
    ++g_fail;
  }

  bool wrote = false;
  for (uint8_t x : L) wrote |= x != 9;
  for (uint8_t x : R) wrote |= x != 9;
  for (uint8_t x : OL) wrote |= x != 9;
  for (uint8_t x : OR_) wrote |= x != 9;
  for (uint8_t x : V) wrote |= x != 9;
  for (float x : C) wrote |= x != -7.f;
  for (float x : MI) wrote |= x != -7.f;
  for (float x : MO) wrote |= x != -7.f;
  if (wrote) {
    std::printf("FAIL a refused call wrote to a buffer\n");
    ++g_fail;
  }
  if (g_fail)
    std::printf("FAIL rectify: %d failed checks\n", g_fail);
  else
    std::printf("OK: 0 failed checks\n");
  return g_fail ? 1 : 0;
}
