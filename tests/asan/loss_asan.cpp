// Host-side AddressSanitizer run of the edge-aware loss's three entries (lea_median5x5_f32,
// lea_edge_loss_f32, lea_edge_loss_grad_f32), built and run by `make asan` after the other
// three drivers, the same way: every csrc unit with ASan on its host side, nothing launched.
// Each refused call must return LEA_E_INVALID, leave a lea_last_error() that names the
// entry, and touch none of its buffers.
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
  // B = 2, H = 6, W = 7: a map is 84 floats; host memory, the checks never dereference it
  constexpr int kHW = 42, kMap = 2 * kHW;
  static float buf[5 * kMap];
  static double sums[4 + 16];  // the sums, then a workspace of two workgroups' partials
  static float scales[2] = {1.f, 0.2f};
  for (float& v : buf) v = -7.f;
  for (double& v : sums) v = -7.0;
  float *pred = buf, *target = buf + kMap, *ts = buf + 2 * kMap, *out = buf + 3 * kMap;
  double* ws = sums + 4;
  if (lea_edge_loss_workspace_bytes(2, 6, 7) != 2 * 4 * sizeof(double) || lea_edge_loss_workspace_bytes(2, 0, 7) != 0) {
    std::printf("FAIL lea_edge_loss_workspace_bytes\n");
    ++g_fail;
  }
  {
    const char* who = "lea_median5x5_f32";
    auto call = [&](const float* x, int64_t xbs, float* y, int64_t ybs, int B, int H, int W, int it) {
      return lea_median5x5_f32(x, xbs, y, ybs, B, H, W, it, nullptr);
    };
    expect_err(who, "null x", call(nullptr, kHW, out, kHW, 2, 6, 7, 2), LEA_E_INVALID);
    expect_err(who, "null y", call(pred, kHW, nullptr, kHW, 2, 6, 7, 2), LEA_E_INVALID);
    expect_err(who, "iterations 0", call(pred, kHW, out, kHW, 2, 6, 7, 0), LEA_E_INVALID);
    expect_err(who, "iterations 3", call(pred, kHW, out, kHW, 2, 6, 7, 3), LEA_E_INVALID);
    expect_err(who, "x stride below H*W", call(pred, kHW - 1, out, kHW, 2, 6, 7, 1), LEA_E_INVALID);
    expect_err(who, "y stride below H*W", call(pred, kHW, out, 0, 2, 6, 7, 1), LEA_E_INVALID);
    expect_err(who, "B = 0", call(pred, kHW, out, kHW, 0, 6, 7, 1), LEA_E_INVALID);
    expect_err(who, "H < 0", call(pred, kHW, out, kHW, 2, -6, 7, 1), LEA_E_INVALID);
    expect_err(who, "W = 0", call(pred, kHW, out, kHW, 2, 6, 0, 1), LEA_E_INVALID);
    expect_err(who, "in place", call(pred, kHW, pred, kHW, 2, 6, 7, 2), LEA_E_INVALID);
    expect_err(who, "y starts in x's last element", call(pred, kHW, pred + kMap - 1, kHW, 2, 6, 7, 2), LEA_E_INVALID);
    expect_err(who, "x starts in y's last element", call(out + kMap - 1, kHW, out, kHW, 2, 6, 7, 2), LEA_E_INVALID);
  }
  {
    const char* who = "lea_edge_loss_f32";
    auto call = [&](const float* p, const float* t, const float* s, int64_t bs, int B, int H, int W, float md,
                    double* su, void* w) {
      return lea_edge_loss_f32(p, bs, t, bs, s, bs, B, H, W, md, su, w, nullptr);
    };
    expect_err(who, "null pred", call(nullptr, target, ts, kHW, 2, 6, 7, 48.f, sums, ws), LEA_E_INVALID);
    expect_err(who, "null target", call(pred, nullptr, ts, kHW, 2, 6, 7, 48.f, sums, ws), LEA_E_INVALID);
    expect_err(who, "null tsmooth", call(pred, target, nullptr, kHW, 2, 6, 7, 48.f, sums, ws), LEA_E_INVALID);
    expect_err(who, "null sums", call(pred, target, ts, kHW, 2, 6, 7, 48.f, nullptr, ws), LEA_E_INVALID);
    expect_err(who, "null workspace", call(pred, target, ts, kHW, 2, 6, 7, 48.f, sums, nullptr), LEA_E_INVALID);
    expect_err(who, "H = 2", call(pred, target, ts, kHW, 2, 2, 7, 48.f, sums, ws), LEA_E_INVALID);
    expect_err(who, "W = 2", call(pred, target, ts, kHW, 2, 6, 2, 48.f, sums, ws), LEA_E_INVALID);
    expect_err(who, "B = 0", call(pred, target, ts, kHW, 0, 6, 7, 48.f, sums, ws), LEA_E_INVALID);
    expect_err(who, "stride below H*W", call(pred, target, ts, kHW - 1, 2, 6, 7, 48.f, sums, ws), LEA_E_INVALID);
    expect_err(who, "maxdisp NaN", call(pred, target, ts, kHW, 2, 6, 7, std::nanf(""), sums, ws), LEA_E_INVALID);
    expect_err(who, "misaligned sums",
               call(pred, target, ts, kHW, 2, 6, 7, 48.f, (double*)((char*)sums + 4), ws), LEA_E_INVALID);
    expect_err(who, "workspace inside sums", call(pred, target, ts, kHW, 2, 6, 7, 48.f, sums, sums + 3), LEA_E_INVALID);
  }
  {
    const char* who = "lea_edge_loss_grad_f32";
    auto call = [&](const float* p, const float* t, const float* s, int64_t bs, const double* su, const float* sc,
                    float* d, int64_t dbs, int B, int H, int W, float md) {
      return lea_edge_loss_grad_f32(p, bs, t, bs, s, bs, su, sc, d, dbs, B, H, W, md, nullptr);
    };
    expect_err(who, "null pred", call(nullptr, target, ts, kHW, sums, scales, out, kHW, 2, 6, 7, 48.f), LEA_E_INVALID);
    expect_err(who, "null sums", call(pred, target, ts, kHW, nullptr, scales, out, kHW, 2, 6, 7, 48.f), LEA_E_INVALID);
    expect_err(who, "null scales", call(pred, target, ts, kHW, sums, nullptr, out, kHW, 2, 6, 7, 48.f), LEA_E_INVALID);
    expect_err(who, "null dpred", call(pred, target, ts, kHW, sums, scales, nullptr, kHW, 2, 6, 7, 48.f),
               LEA_E_INVALID);
    expect_err(who, "H = 2", call(pred, target, ts, kHW, sums, scales, out, kHW, 2, 2, 7, 48.f), LEA_E_INVALID);
    expect_err(who, "W = 1", call(pred, target, ts, kHW, sums, scales, out, kHW, 2, 6, 1, 48.f), LEA_E_INVALID);
    expect_err(who, "dpred stride below H*W", call(pred, target, ts, kHW, sums, scales, out, kHW - 1, 2, 6, 7, 48.f),
               LEA_E_INVALID);
    expect_err(who, "maxdisp NaN", call(pred, target, ts, kHW, sums, scales, out, kHW, 2, 6, 7, std::nanf("")),
               LEA_E_INVALID);
    expect_err(who, "dpred = pred", call(pred, target, ts, kHW, sums, scales, pred, kHW, 2, 6, 7, 48.f), LEA_E_INVALID);
    expect_err(who, "dpred starts in target's last element",
               call(pred, target, ts, kHW, sums, scales, target + kMap - 1, kHW, 2, 6, 7, 48.f), LEA_E_INVALID);
    expect_err(who, "tsmooth starts in dpred's last element",
               call(pred, target, out + kMap - 1, kHW, sums, scales, out, kHW, 2, 6, 7, 48.f), LEA_E_INVALID);
    expect_err(who, "dpred over the scales", call(pred, target, ts, kHW, sums, scales, scales + 1, kHW, 2, 6, 7, 48.f),
               LEA_E_INVALID);
  }
  for (float v : buf)
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
  if (scales[0] != 1.f || scales[1] != 0.2f) {
    std::printf("FAIL a refused call wrote to the scales\n");
    ++g_fail;
  }
  std::printf("%s loss: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
