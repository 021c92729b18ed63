// Host-side AddressSanitizer run of the view synthesis entry (lea_forward_warp_f32), built and
// run by `make asan` after the other eleven drivers, the same way: every csrc unit with ASan on
// its host side, nothing launched.  Each refused call must return LEA_E_INVALID, leave a
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
  // B = 2, C = 3, H = 4, W = 6: a plane is 24 floats, the image 144, a [B, H, W] map 48; host
  // memory, the checks never dereference it
  constexpr int B = 2, C = 3, H = 4, W = 6, kPlane = H * W, kMap = B * kPlane, kImg = C * kMap;
  static float img[kImg], disp[kMap], scales[B], warped[kImg], zview[kMap], source[kMap], spare[kImg];
  static uint8_t excl[kMap], state[kMap];
  float* fbufs[] = {img, disp, scales, warped, zview, source, spare};
  const size_t flen[] = {kImg, kMap, B, kImg, kMap, kMap, kImg};
  for (int i = 0; i < 7; ++i)
    for (size_t j = 0; j < flen[i]; ++j) fbufs[i][j] = -7.f;
  for (uint8_t& v : excl) v = 9;
  for (uint8_t& v : state) v = 9;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  const char* who = "lea_forward_warp_f32";
  struct Args {
    const float* image;
    int64_t ibs;
    const float* disp;
    int64_t dbs;
    const uint8_t* exclude;
    const float* scales;
    int B, C, H, W;
    float max_diff, max_stretch;
    int fill;
    float* warped;
    float* zview;
    uint8_t* state;
    float* source;
  };
  const Args good = {img, C * kPlane, disp, kPlane, excl, scales, B, C, H, W, 1.f, 4.f, 1, warped, zview, state, source};
  auto call = [&](const Args& a) {
    return lea_forward_warp_f32(a.image, a.ibs, a.disp, a.dbs, a.exclude, a.scales, a.B, a.C, a.H, a.W, a.max_diff,
                                a.max_stretch, a.fill, 0.f, a.warped, a.zview, a.state, a.source, nullptr);
  };
  auto refuse = [&](const char* what, Args a) { expect_err(who, what, call(a), LEA_E_INVALID); };
  Args a;
  // null required pointers, all outputs null
  a = good; a.image = nullptr; refuse("null image", a);
  a = good; a.disp = nullptr; refuse("null disp", a);
  a = good; a.scales = nullptr; refuse("null scales", a);
  a = good; a.warped = nullptr; a.zview = nullptr; a.state = nullptr; a.source = nullptr; refuse("all outputs null", a);
  // sizes and limits
  a = good; a.B = 0; refuse("B = 0", a);
  a = good; a.H = -4; refuse("H < 0", a);
  a = good; a.W = 0; refuse("W = 0", a);
  a = good; a.W = LEA_FORWARD_WARP_MAX_W + 1; a.ibs = (int64_t)C * H * a.W; a.dbs = (int64_t)H * a.W;
  refuse("W above the limit", a);
  a = good; a.B = 65536; a.H = 65536; refuse("B*H above 2^31 - 1", a);
  a = good; a.C = 0; refuse("C = 0", a);
  a = good; a.C = 5; a.ibs = 5 * kPlane; refuse("C = 5", a);
  // batch strides below the block
  a = good; a.ibs = C * kPlane - 1; refuse("image stride below C*H*W", a);
  a = good; a.ibs = -1; refuse("image stride negative", a);
  a = good; a.dbs = kPlane - 1; refuse("disp stride below H*W", a);
  a = good; a.dbs = 0; refuse("disp stride 0", a);
  // max_diff, max_stretch, fill
  a = good; a.max_diff = -0.5f; refuse("max_diff < 0", a);
  a = good; a.max_diff = nan; refuse("max_diff NaN", a);
  a = good; a.max_diff = inf; refuse("max_diff inf", a);
  a = good; a.max_stretch = 0.5f; refuse("max_stretch < 1", a);
  a = good; a.max_stretch = 64.5f; refuse("max_stretch > 64", a);
  a = good; a.max_stretch = nan; refuse("max_stretch NaN", a);
  a = good; a.max_stretch = inf; refuse("max_stretch inf", a);
  a = good; a.fill = 2; refuse("fill = 2", a);
  // every output against every input, scales and every other output
  a = good; a.warped = img; refuse("warped = image", a);
  a = good; a.warped = img + kImg - 1; refuse("warped starts in the image's last element", a);
  a = good; a.image = warped + kImg - 1; refuse("image starts in warped's last element", a);
  a = good; a.warped = spare; a.disp = spare + kImg - 1; refuse("disp starts in warped's last element", a);
  a = good; a.zview = disp; refuse("zview = disp", a);
  a = good; a.zview = (float*)scales; a.B = 1; refuse("zview over scales", a);
  a = good; a.source = (float*)scales - kMap + 1; refuse("source ends in scales' first element", a);
  a = good; a.state = (uint8_t*)excl; refuse("state = exclude", a);
  a = good; a.state = (uint8_t*)excl + kMap - 1; refuse("state starts in exclude's last byte", a);
  a = good; a.state = (uint8_t*)img; refuse("state inside image", a);
  a = good; a.state = (uint8_t*)(disp + kMap) - 1; refuse("state starts in disp's last byte", a);
  a = good; a.source = zview; refuse("source = zview", a);
  a = good; a.source = zview + kMap - 1; refuse("source starts in zview's last element", a);
  a = good; a.zview = warped + kImg - 1; refuse("zview starts in warped's last element", a);
  a = good; a.state = (uint8_t*)(warped + kImg) - 1; refuse("state starts in warped's last byte", a);
  a = good; a.state = (uint8_t*)source; refuse("state inside source", a);
  a = good; a.state = (uint8_t*)zview + 4 * kMap - 1; refuse("state starts in zview's last byte", a);
  // a strided image reaches further than a packed one: the span counts the stride
  a = good; a.C = 1; a.image = spare; a.ibs = kImg - kPlane; a.warped = spare + kImg - 1;
  refuse("warped in the strided image's last element", a);
  // outputs that are not wanted are not looked at
  a = good; a.warped = nullptr; a.zview = nullptr; a.source = nullptr; a.state = (uint8_t*)excl;
  refuse("state alone, over exclude", a);

  for (int i = 0; i < 7; ++i)
    for (size_t j = 0; j < flen[i]; ++j)
      if (fbufs[i][j] != -7.f) {
        std::printf("FAIL a refused call wrote to float buffer %d\n", i);
        ++g_fail;
        i = 7;
        break;
      }
  for (int i = 0; i < kMap; ++i)
    if (excl[i] != 9 || state[i] != 9) {
      std::printf("FAIL a refused call wrote to the byte buffers\n");
      ++g_fail;
      break;
    }
  std::printf("%s warp: %d failed checks\n", g_fail ? "FAIL" : "OK", g_fail);
  return g_fail ? 1 : 0;
}
