// Rectification of a raw stereo pair: both views of a batch in one launch, from a calibration
// block in device memory (the map is computed per pixel) or from given maps, bilinear, uint8 in
// and out.  The definition is at lea_rectify_pair_u8 in include/leastereo_hip.h.
//
// A lane owns kRectPer consecutive pixels of one output row: their source coordinates (rect_map,
// contraction off, the order of tests/rectify_judge.py), then rect_pixel, the one copy of the
// pixel stage for computed and given maps.  The lane's ps * kRectPer bytes are packed into
// dwords and stored with rect_store_span: whole dwords where the span is 4-byte aligned, else a
// byte head, funnel-shifted aligned dwords and a byte tail (a row of a 3-byte image starts on a
// dword only for some widths; the misalignment is the same for every lane of a row).  The taps
// are byte gathers: neighbouring lanes read neighbouring source bytes, so they come from the
// vector L1 and the L2.  No value is converted to an integer, and no address formed from it,
// before the validity test has bounded it.
#include <cmath>

#include "common.h"

namespace lea {

constexpr int kRectThreads = 256;
constexpr int kRectPer = 4;  // pixels of a lane, consecutive in x
// workgroup tile: TX lanes along x (TX * kRectPer pixels) by kRectThreads / TX rows
constexpr int kRectSquareTX = 32;  // 128 x 8 pixels
constexpr int kRectRowTX = 256;    // 1024 x 1 pixels
constexpr int kRectCalFloats = 24;

static std::atomic<int> g_rect_tile{0};  // lea_rectify_set_tile

// the source coordinates of the rectified pixel (u, v) of one view: c is the view's 24 floats
__device__ __forceinline__ void rect_map(const float* __restrict__ c, float u, float v, float& sx, float& sy) {
#pragma clang fp contract(off)
  const float X = (c[0] * u + c[1] * v) + c[2];
  const float Y = (c[3] * u + c[4] * v) + c[5];
  const float Wc = (c[6] * u + c[7] * v) + c[8];
  const float nan = __builtin_nanf("");
  if (!(Wc > 0.f)) {
    sx = sy = nan;
    return;
  }
  const float x = X / Wc, y = Y / Wc;
  const float xx = x * x, yy = y * y;
  const float r2 = xx + yy;
  const float* k = c + 14;
  float xd, yd;
  if (c[13] == 1.f) {  // fisheye (equidistant)
    const float r = sqrtf(r2);
    const float th = atanf(r);
    const float t2 = th * th;
    const float thd = th * (1.f + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
    const float s = r > 1e-8f ? thd / r : 1.f;
    xd = x * s;
    yd = y * s;
  } else {  // pinhole, rational: k1 k2 p1 p2 k3 k4 k5 k6
    const float num = 1.f + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
    const float den = 1.f + r2 * (k[5] + r2 * (k[6] + r2 * k[7]));
    const float rad = num / den;
    const float xy = x * y;
    const float tx = (2.f * k[2]) * xy + k[3] * (r2 + 2.f * xx);
    const float ty = k[2] * (r2 + 2.f * yy) + (2.f * k[3]) * xy;
    xd = x * rad + tx;
    yd = y * rad + ty;
  }
  sx = c[9] * xd + c[11];
  sy = c[10] * yd + c[12];
}

// the pixel stage: the PS bytes of the output pixel whose source coordinates are (sx, sy), as
// the low PS bytes of the result, and its validity
template <int PS>
__device__ __forceinline__ unsigned rect_pixel(const unsigned char* __restrict__ img, int H, int W, float sx, float sy,
                                               unsigned fill, bool& ok) {
#pragma clang fp contract(off)
  ok = sx >= 0.f && sx <= (float)(W - 1) && sy >= 0.f && sy <= (float)(H - 1);  // NaN fails
  if (!ok) return fill;
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const int x0 = (int)fx0, y0 = (int)fy0;  // in 0 .. W - 1, 0 .. H - 1
  const float ax = sx - fx0, ay = sy - fy0;
  const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
  const unsigned char* r0 = img + (size_t)y0 * (size_t)W * PS;
  const unsigned char* r1 = img + (size_t)y1 * (size_t)W * PS;
  const unsigned char *pa = r0 + (size_t)x0 * PS, *pb = r0 + (size_t)x1 * PS;
  const unsigned char *pc = r1 + (size_t)x0 * PS, *pd = r1 + (size_t)x1 * PS;
  unsigned out = 0;
#pragma unroll
  for (int ch = 0; ch < PS; ++ch) {
    const float a = (float)pa[ch], b = (float)pb[ch], c = (float)pc[ch], d = (float)pd[ch];
    const float top = a + ax * (b - a);
    const float bot = c + ax * (d - c);
    const float v = top + ay * (bot - top);
    out |= ((unsigned)(int)rintf(v) & 0xffu) << (8 * ch);  // v in [0, 255]; half to even
  }
  return out;
}

// 4 * NW bytes, little-endian in w, to p: dwords when p is 4-byte aligned, else a byte head, the
// aligned dwords in between and a byte tail
template <int NW>
__device__ __forceinline__ void rect_store_span(unsigned char* __restrict__ p, const unsigned (&w)[NW]) {
  const unsigned m = (unsigned)((uintptr_t)p & 3);
  if (m == 0) {
    unsigned* q = reinterpret_cast<unsigned*>(p);
#pragma unroll
    for (int j = 0; j < NW; ++j) q[j] = w[j];
    return;
  }
  const unsigned s = 4 - m;  // head bytes, 1 .. 3
  for (unsigned i = 0; i < s; ++i) p[i] = (unsigned char)(w[0] >> (8 * i));
  unsigned* q = reinterpret_cast<unsigned*>(p + s);
#pragma unroll
  for (int j = 0; j + 1 < NW; ++j) q[j] = (w[j] >> (8 * s)) | (w[j + 1] << (8 * m));
  for (unsigned i = 0; i < m; ++i) p[s + 4 * (NW - 1) + i] = (unsigned char)(w[NW - 1] >> (8 * (s + i)));
}

template <int PS, int TX>
__global__ __launch_bounds__(kRectThreads) void rectify_pair_kernel(
    const unsigned char* __restrict__ left, const unsigned char* __restrict__ right, int H, int W,
    const float* __restrict__ calib, long long calib_bstride, const float* __restrict__ maps_in,
    long long maps_bstride, int Ho, int Wo, unsigned fill, unsigned char* __restrict__ out_left,
    unsigned char* __restrict__ out_right, unsigned char* __restrict__ valid, float* __restrict__ maps_out) {
  constexpr int TY = kRectThreads / TX;
  const int view = (int)(blockIdx.z & 1u), b = (int)(blockIdx.z >> 1);
  const int tx = (int)threadIdx.x % TX, ty = (int)threadIdx.x / TX;
  const int x0 = ((int)blockIdx.x * TX + tx) * kRectPer;
  const int y = (int)blockIdx.y * TY + ty;
  if (y >= Ho || x0 >= Wo) return;
  const int n = Wo - x0 < kRectPer ? Wo - x0 : kRectPer;  // pixels of this lane
  const size_t hwo = (size_t)Ho * (size_t)Wo;
  const size_t row = (size_t)y * (size_t)Wo + (size_t)x0;  // first pixel within a plane
  const unsigned char* img = (view ? right : left) + (size_t)b * (size_t)H * (size_t)W * PS;

  float sx[kRectPer], sy[kRectPer];
  if (maps_in) {
    const float* mx = maps_in + (size_t)b * (size_t)maps_bstride + (size_t)(2 * view) * hwo + row;
    const float* my = mx + hwo;
#pragma unroll
    for (int j = 0; j < kRectPer; ++j) {
      sx[j] = j < n ? mx[j] : 0.f;
      sy[j] = j < n ? my[j] : 0.f;
    }
  } else {
    const float* c = calib + (size_t)b * (size_t)calib_bstride + view * kRectCalFloats;
    const float v = (float)y;
#pragma unroll
    for (int j = 0; j < kRectPer; ++j) rect_map(c, (float)(x0 + j), v, sx[j], sy[j]);
  }

  unsigned px[kRectPer];
  unsigned okbits = 0;
#pragma unroll
  for (int j = 0; j < kRectPer; ++j) {
    bool ok = false;
    px[j] = j < n ? rect_pixel<PS>(img, H, W, sx[j], sy[j], fill, ok) : 0u;
    okbits |= (ok ? 1u : 0u) << (8 * j);
  }

  const size_t pix = ((size_t)b * hwo + row);
  unsigned char* o = (view ? out_right : out_left) + pix * PS;
  if (n == kRectPer) {
    if (PS == 4) {
      const unsigned w[4] = {px[0], px[1], px[2], px[3]};
      rect_store_span<4>(o, w);
    } else {
      const unsigned w[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
      rect_store_span<3>(o, w);
    }
  } else {
    for (int j = 0; j < n; ++j)
#pragma unroll
      for (int ch = 0; ch < PS; ++ch) o[j * PS + ch] = (unsigned char)(px[j] >> (8 * ch));
  }
  if (valid) {
    unsigned char* vp = valid + ((size_t)(2 * b + view) * hwo + row);
    if (n == kRectPer) {
      const unsigned w[1] = {okbits};
      rect_store_span<1>(vp, w);
    } else {
      for (int j = 0; j < n; ++j) vp[j] = (unsigned char)(okbits >> (8 * j));
    }
  }
  if (maps_out) {
    float* mx = maps_out + ((size_t)(2 * b + view) * 2) * hwo + row;
    float* my = mx + hwo;
#pragma unroll
    for (int j = 0; j < kRectPer; ++j)
      if (j < n) {
        mx[j] = sx[j];
        my[j] = sy[j];
      }
  }
}

template <int PS, int TX>
static void rect_launch(hipStream_t s, int B, const unsigned char* l, const unsigned char* r, int H, int W,
                        const float* calib, long long cbs, const float* maps_in, long long mbs, int Ho, int Wo,
                        unsigned fill, unsigned char* ol, unsigned char* orr, unsigned char* valid, float* maps_out) {
  constexpr int TY = kRectThreads / TX;
  const dim3 grid((unsigned)((Wo + TX * kRectPer - 1) / (TX * kRectPer)), (unsigned)((Ho + TY - 1) / TY),
                  (unsigned)(2 * B));
  rectify_pair_kernel<PS, TX><<<grid, kRectThreads, 0, s>>>(l, r, H, W, calib, cbs, maps_in, mbs, Ho, Wo, fill, ol,
                                                            orr, valid, maps_out);
}

}  // namespace lea

extern "C" int lea_rectify_set_tile(int mode) {
  lea::clear_error();
  LEA_CHECK_ARG(mode == 0 || mode == 1, "lea_rectify_set_tile: mode %d is not 0 or 1", mode);
  lea::g_rect_tile.store(mode, std::memory_order_relaxed);
  return LEA_OK;
}
LEA_TUNING_HOOK(lea_rectify_set_tile, 1, v[0] = lea::g_rect_tile.load(std::memory_order_relaxed))

extern "C" int lea_rectify_pair_u8(const void* left, const void* right, int pix_stride, int B, int H, int W,
                                   const float* calib, int Bc, const float* maps_in, int Bm, int Ho, int Wo, int fill,
                                   void* out_left, void* out_right, uint8_t* valid, float* maps_out, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_rectify_pair_u8";
  LEA_CHECK_ARG(left && right, "%s: left or right is null", who);
  LEA_CHECK_ARG(out_left && out_right, "%s: out_left or out_right is null", who);
  LEA_CHECK_ARG(pix_stride == 3 || pix_stride == 4, "%s: pix_stride %d is not 3 or 4", who, pix_stride);
  LEA_CHECK_ARG(B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "%s: bad shape B=%d H=%d W=%d Ho=%d Wo=%d", who, B, H, W,
                Ho, Wo);
  LEA_CHECK_ARG(B <= 32767 && H <= 65535 && W <= 65535 && Ho <= 65535 && Wo <= 65535,
                "%s: B=%d above 32767, or one of H=%d W=%d Ho=%d Wo=%d above 65535", who, B, H, W, Ho, Wo);
  LEA_CHECK_ARG((calib != nullptr) != (maps_in != nullptr), "%s: exactly one of calib and maps_in must be given (%s)",
                who, calib ? "both are" : "neither is");
  if (calib) LEA_CHECK_ARG(Bc == 1 || Bc == B, "%s: calib batch %d is neither 1 nor B=%d", who, Bc, B);
  if (maps_in) LEA_CHECK_ARG(Bm == 1 || Bm == B, "%s: maps_in batch %d is neither 1 nor B=%d", who, Bm, B);
  LEA_CHECK_ARG(fill >= 0 && fill <= 255, "%s: fill %d outside 0..255", who, fill);
  LEA_CHECK_ARG((((uintptr_t)calib | (uintptr_t)maps_in | (uintptr_t)maps_out) & 3) == 0,
                "%s: calib, maps_in and maps_out must be 4-byte aligned", who);
  const size_t ps = (size_t)pix_stride;
  const size_t hw = (size_t)H * (size_t)W, hwo = (size_t)Ho * (size_t)Wo;
  {  // no output may overlap an input or another output
    const void* ins[4] = {left, right, calib, maps_in};
    const size_t inn[4] = {(size_t)B * hw * ps, (size_t)B * hw * ps, calib ? (size_t)Bc * 2 * kRectCalFloats * 4 : 0,
                           maps_in ? (size_t)Bm * 4 * hwo * 4 : 0};
    const char* inname[4] = {"left", "right", "calib", "maps_in"};
    const void* outs[4] = {out_left, out_right, valid, maps_out};
    const size_t outn[4] = {(size_t)B * hwo * ps, (size_t)B * hwo * ps, (size_t)B * 2 * hwo, (size_t)B * 4 * hwo * 4};
    const char* outname[4] = {"out_left", "out_right", "valid", "maps_out"};
    for (int o = 0; o < 4; ++o) {
      if (!outs[o]) continue;
      for (int i = 0; i < 4; ++i)
        LEA_CHECK_ARG(!ins[i] || !spans_overlap(outs[o], outn[o], ins[i], inn[i]), "%s: %s overlaps %s", who,
                      outname[o], inname[i]);
      for (int q = 0; q < o; ++q)
        LEA_CHECK_ARG(!outs[q] || !spans_overlap(outs[o], outn[o], outs[q], outn[q]), "%s: %s overlaps %s", who,
                      outname[o], outname[q]);
    }
  }
  const unsigned char* l = static_cast<const unsigned char*>(left);
  const unsigned char* r = static_cast<const unsigned char*>(right);
  unsigned char* ol = static_cast<unsigned char*>(out_left);
  unsigned char* orr = static_cast<unsigned char*>(out_right);
  const long long cbs = calib && Bc == B ? 2 * kRectCalFloats : 0;
  const long long mbs = maps_in && Bm == B ? (long long)(4 * hwo) : 0;
  unsigned f = (unsigned)fill;
  f |= f << 8;
  f |= f << 16;
  if (pix_stride == 3) f &= 0xffffffu;
  hipStream_t s = as_stream(stream);
  const bool rowtile = g_rect_tile.load(std::memory_order_relaxed) == 1;
#define LEA_RECT_GO(PS, TX) \
  rect_launch<PS, TX>(s, B, l, r, H, W, calib, cbs, maps_in, mbs, Ho, Wo, f, ol, orr, valid, maps_out)
  if (pix_stride == 3) {
    if (rowtile)
      LEA_RECT_GO(3, kRectRowTX);
    else
      LEA_RECT_GO(3, kRectSquareTX);
  } else {
    if (rowtile)
      LEA_RECT_GO(4, kRectRowTX);
    else
      LEA_RECT_GO(4, kRectSquareTX);
  }
#undef LEA_RECT_GO
  return launch_status(who);
}
