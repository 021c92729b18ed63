// Host-side AddressSanitizer run of lea_disparity_regression_stats' argument checks
// (built and run by `make asan` after capi_asan, the same way: every csrc unit with ASan
// on its host side, nothing launched).  Each refused call must return the documented
// code, leave a lea_last_error() that names the entry, and touch none of its buffers.
// Exit 0 = every check passed and ASan saw no error.
#include <cstdio>
#include <cstring>

#include "leastereo_hip.h"

static int g_fail = 0;
static const char kEntry[] = "lea_disparity_regression_stats";

static void expect_err(const char* what, int rc, int want) {
  const char* e = lea_last_error();
  if (rc != want || e == nullptr || std::strstr(e, kEntry) == nullptr) {
    std::printf("FAIL %s: rc=%d (want %d) err='%s'\n", what, rc, want, e ? e : "(null)");
    ++g_fail;
  }
}

int main() {
  if (lea_abi_version() < 14) {
    std::printf("FAIL abi version %d\n", lea_abi_version());
    ++g_fail;
  }
  // B = 1, D3 = 4, H3 = 2, W3 = 2: cost 16 floats, every output 36 floats; host memory, the
  // checks never dereference it
  constexpr int kOut = 36;
  static float cost[16], out[4 * kOut];
  float *disp = out, *ent = out + kOut, *peak = out + 2 * kOut, *loc = out + 3 * kOut;
  for (float& v : out) v = -7.f;
  auto call = [&](const void* c, float* d, float* e, float* p, float* l, int B, int D3, int H3, int W3, int md,
                  int r, int dt) { return lea_disparity_regression_stats(c, d, e, p, l, B, D3, H3, W3, md, r, dt, nullptr); };
  expect_err("null cost", call(nullptr, disp, ent, peak, loc, 1, 4, 2, 2, 12, 4, LEA_F32), LEA_E_INVALID);
  expect_err("null disp", call(cost, nullptr, ent, peak, loc, 1, 4, 2, 2, 12, 4, LEA_F32), LEA_E_INVALID);
  expect_err("no optional output", call(cost, disp, nullptr, nullptr, nullptr, 1, 4, 2, 2, 12, 4, LEA_F32),
             LEA_E_INVALID);
  expect_err("B = 0", call(cost, disp, ent, peak, loc, 0, 4, 2, 2, 12, 4, LEA_F32), LEA_E_INVALID);
  expect_err("D3 < 0", call(cost, disp, ent, peak, loc, 1, -4, 2, 2, 12, 4, LEA_F32), LEA_E_INVALID);
  expect_err("H3 = 0", call(cost, disp, ent, peak, loc, 1, 4, 0, 2, 12, 4, LEA_F32), LEA_E_INVALID);
  expect_err("W3 = 0", call(cost, disp, ent, peak, loc, 1, 4, 2, 0, 12, 4, LEA_F32), LEA_E_INVALID);
  expect_err("maxdisp = 0", call(cost, disp, ent, peak, loc, 1, 4, 2, 2, 0, 4, LEA_F32), LEA_E_INVALID);
  expect_err("radius 0", call(cost, disp, ent, peak, loc, 1, 4, 2, 2, 12, 0, LEA_F32), LEA_E_INVALID);
  expect_err("radius 17", call(cost, disp, ent, peak, loc, 1, 4, 2, 2, 12, 17, LEA_F32), LEA_E_INVALID);
  expect_err("dtype", call(cost, disp, ent, peak, loc, 1, 4, 2, 2, 12, 4, 7), LEA_E_UNSUPPORTED);
  expect_err("maxdisp != 3 D3", call(cost, disp, ent, peak, loc, 1, 4, 2, 2, 13, 4, LEA_F32), LEA_E_UNSUPPORTED);
  expect_err("maxdisp 2 D3", call(cost, disp, ent, peak, loc, 1, 4, 2, 2, 8, 4, LEA_BF16), LEA_E_UNSUPPORTED);
  expect_err("entropy = disp", call(cost, disp, disp, peak, loc, 1, 4, 2, 2, 12, 4, LEA_F32), LEA_E_INVALID);
  expect_err("peak overlaps entropy", call(cost, disp, ent, ent + kOut - 1, loc, 1, 4, 2, 2, 12, 4, LEA_F32),
             LEA_E_INVALID);
  expect_err("local = peak, entropy null", call(cost, disp, nullptr, peak, peak, 1, 4, 2, 2, 12, 4, LEA_F32),
             LEA_E_INVALID);
  expect_err("disp = cost", call(out, out, ent, peak, loc, 1, 4, 2, 2, 12, 4, LEA_F32), LEA_E_INVALID);
  expect_err("local inside cost", call(out, disp + kOut, nullptr, nullptr, out + 15, 1, 4, 2, 2, 12, 4, LEA_F32),
             LEA_E_INVALID);
  for (float v : out)
    if (v != -7.f) {
      std::printf("FAIL a refused call wrote to a buffer\n");
      ++g_fail;
      break;
    }
  std::printf("%s disp_stats: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
