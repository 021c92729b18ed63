// Host-side AddressSanitizer run of the disparity refinement's two entries
// (lea_disparity_refine_workspace_bytes, lea_disparity_refine_f32), built and run by
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
  expect_bytes("2x6x7", lea_disparity_refine_workspace_bytes(2, 6, 7), 7 * 4 * 84);
  expect_bytes("1x1x1", lea_disparity_refine_workspace_bytes(1, 1, 1), 28);
  expect_bytes("1x2048x2048", lea_disparity_refine_workspace_bytes(1, 2048, 2048), (size_t)28 << 22);
  expect_bytes("B = 0", lea_disparity_refine_workspace_bytes(0, 6, 7), 0);
  expect_bytes("H < 0", lea_disparity_refine_workspace_bytes(2, -6, 7), 0);
  expect_bytes("W = 0", lea_disparity_refine_workspace_bytes(2, 6, 0), 0);

  // B = 2, C = 3, H = 6, W = 7: a map is 84 floats, the guide 252, the workspace 588; host
  // memory, the checks never dereference it
  constexpr int kMap = 84, kGuide = 252, kWs = 588;
  static float guide[kGuide + kMap], disp[kMap], conf[kMap], ws[kWs + kMap], out[kMap], sup[kMap];
  static uint8_t ex[kMap];
  float* all[6] = {guide, disp, conf, ws, out, sup};
  const int alln[6] = {kGuide + kMap, kMap, kMap, kWs + kMap, kMap, kMap};
  for (int i = 0; i < 6; ++i)
    for (int k = 0; k < alln[i]; ++k) all[i][k] = -7.f;
  for (uint8_t& v : ex) v = 9;
  const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();
  const char* who = "lea_disparity_refine_f32";
  auto call = [&](const float* g, int64_t gbs, const float* d, const float* c, const uint8_t* e, int B, int C, int H,
                  int W, float lam, float sig, int T, void* w, float* o, float* s) {
    return lea_disparity_refine_f32(g, gbs, d, c, e, B, C, H, W, lam, sig, T, w, o, s, nullptr);
  };
  expect_err(who, "null guide", call(nullptr, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "null disp", call(guide, 126, nullptr, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "null workspace", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, nullptr, out, sup),
             LEA_E_INVALID);
  expect_err(who, "null refined", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, nullptr, sup),
             LEA_E_INVALID);
  expect_err(who, "B = 0", call(guide, 126, disp, conf, ex, 0, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "H < 0", call(guide, 126, disp, conf, ex, 2, 3, -6, 7, 8000.f, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "W = 0", call(guide, 126, disp, conf, ex, 2, 3, 6, 0, 8000.f, 0.05f, 3, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "B too large", call(guide, 126, disp, conf, ex, 32768, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "B*H*W too large",
             call(guide, (int64_t)3 << 40, disp, conf, ex, 2, 3, 1 << 20, 1 << 20, 8000.f, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "C = 0", call(guide, 126, disp, conf, ex, 2, 0, 6, 7, 8000.f, 0.05f, 3, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "C = 5", call(guide, 210, disp, conf, ex, 2, 5, 6, 7, 8000.f, 0.05f, 3, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "T = 0", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 0, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "T = 9", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 9, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "lambda 0", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 0.f, 0.05f, 3, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "lambda < 0", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, -1.f, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "lambda NaN", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, nan, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "lambda inf", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, inf, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "sigma 0", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.f, 3, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "sigma < 0", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, -0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "sigma NaN", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, nan, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "sigma inf", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, inf, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "guide stride below C*H*W",
             call(guide, 125, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, sup), LEA_E_INVALID);
  expect_err(who, "misaligned workspace",
             call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, (char*)ws + 2, out, sup), LEA_E_INVALID);
  expect_err(who, "refined = disp", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, disp, sup),
             LEA_E_INVALID);
  expect_err(who, "refined in the guide's last element",
             call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, guide + kGuide - 1, sup),
             LEA_E_INVALID);
  expect_err(who, "refined in the strided guide's last element",
             call(guide, 168, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, guide + 168 + 125, sup),
             LEA_E_INVALID);
  expect_err(who, "refined = conf", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, conf, sup),
             LEA_E_INVALID);
  expect_err(who, "exclude starts in refined's last byte",
             call(guide, 126, disp, conf, (const uint8_t*)out + 4 * kMap - 1, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, sup),
             LEA_E_INVALID);
  expect_err(who, "refined in the workspace's last element",
             call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, ws + kWs - 1, sup), LEA_E_INVALID);
  expect_err(who, "support = disp", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, disp),
             LEA_E_INVALID);
  expect_err(who, "support = refined", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, out),
             LEA_E_INVALID);
  expect_err(who, "support in the workspace",
             call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, ws, out, ws + 2 * kMap), LEA_E_INVALID);
  expect_err(who, "workspace = conf", call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, conf, out, sup),
             LEA_E_INVALID);
  expect_err(who, "workspace ends in disp",
             call(guide, 126, disp, conf, ex, 2, 3, 6, 7, 8000.f, 0.05f, 3, (void*)((uintptr_t)disp - 4 * (kWs - 1)), out, sup),
             LEA_E_INVALID);
  // the optional ones may be null: the next check in line fires
  expect_err(who, "null conf, exclude, support, then T",
             call(guide, 126, disp, nullptr, nullptr, 2, 3, 6, 7, 8000.f, 0.05f, 0, ws, out, nullptr), LEA_E_INVALID);

  for (int i = 0; i < 6; ++i)
    for (int k = 0; k < alln[i]; ++k)
      if (all[i][k] != -7.f) {
        std::printf("FAIL a refused call wrote to buffer %d\n", i);
        ++g_fail;
        k = alln[i];
      }
  for (uint8_t v : ex)
    if (v != 9) {
      std::printf("FAIL a refused call wrote to the exclude bytes\n");
      ++g_fail;
      break;
    }
  std::printf("%s refine: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
