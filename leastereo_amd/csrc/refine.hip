// Confidence-weighted, image-guided weighted-least-squares refinement of a disparity map by
// the fast global smoother (Min et al. 2014; the scheme behind OpenCV's ximgproc disparity
// WLS filter).  The definition is at lea_disparity_refine_f32 in include/leastereo_hip.h; in
// short: two right-hand sides num = conf * disp and den = conf go through T iterations of a
// horizontal and a vertical pass, each pass solving the tridiagonal systems
// (I + lambda_t L) u = r of every line with the edge weights of the guide, and the result is
// num / den.
//
// Every line is solved by a Thomas sweep held by one lane -- forward elimination, then back
// substitution, the eliminated coefficient -c' and both right-hand sides going through the
// workspace in between -- so the order of operations is fixed and no lane ever waits for
// another.  One kernel does the sweeps, down the first axis of a [B, n, m] plane: a lane owns
// one of the m lines, a wave 64 neighbouring ones, so every load and store is one coalesced
// segment, and the next kFgsU steps' loads are in flight while the current kFgsU are eliminated
// (the loads do not depend on the chain).  The vertical pass is that kernel on the planes as
// they are; the horizontal pass is the same kernel on the transposed planes, with a tiled
// transpose through LDS of num and den before and after it (wh is transposed once per call).
// Launches: the elementwise kernel (evidence and the two weight planes), the transpose of wh,
// then per iteration transpose, sweep, transpose, sweep: 2 + 4 T.  The last vertical sweep
// divides and writes the outputs instead of num and den.
// Plain vector loads and stores only; no atomics, no host copy, no allocation.
#include <cmath>

#include "common.h"

namespace lea {

constexpr int kFgsTile = 32;   // edge of a transpose tile
constexpr int kFgsU = 16;      // rows per register batch of a sweep
constexpr int kFgsPlanes = 7;  // wh (later num transposed), wv, -c', num, den, wh transposed, den transposed
constexpr float kFgsDenMin = 1e-30f;

// evidence (num = c0 * f0, den = c0) and the edge weights to the right and below (0 on the
// last column / row, which makes the end of every line its own special case)
__global__ __launch_bounds__(256) void fgs_init(const float* __restrict__ guide, long long gbs,
                                                const float* __restrict__ disp, const float* __restrict__ conf,
                                                const unsigned char* __restrict__ exclude, int C, int H, int W,
                                                long long n, float sigma, float* __restrict__ wh,
                                                float* __restrict__ wv, float* __restrict__ num,
                                                float* __restrict__ den) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % W);
  const long long row = i / W;
  const int y = (int)(row % H);
  const long long b = row / H;
  const long long hw = (long long)H * W;
  const float* g = guide + b * gbs + (long long)y * W + x;
  float mh = 0.f, mv = 0.f;
  for (int c = 0; c < C; ++c) {
    const float v = g[c * hw];
    if (x < W - 1) mh = fmaxf(mh, fabsf(g[c * hw + 1] - v));
    if (y < H - 1) mv = fmaxf(mv, fabsf(g[c * hw + W] - v));
  }
  wh[i] = x < W - 1 ? expf(-(mh / sigma)) : 0.f;
  wv[i] = y < H - 1 ? expf(-(mv / sigma)) : 0.f;
  const float d = disp[i];
  const float c = conf ? conf[i] : 1.f;
  const bool ok = !(exclude && exclude[i]) && __builtin_isfinite(d) && __builtin_isfinite(c) && c > 0.f;
  const float c0 = ok ? c : 0.f, f0 = ok ? d : 0.f;
  num[i] = c0 * f0;
  den[i] = c0;
}

// One elimination step of a line, in a form without cancellation.  With A = lambda w_(i-1) and
// C = lambda w_i (a_i = -A, c_i = -C, b_i = 1 + A + C) the textbook sweep carries
// c'_i = c_i / (b_i - a_i c'_(i-1)), which tends to -1 as lambda w grows, and what the next
// step needs of it is 1 + c'_i: at lambda w ~ 10^4 that difference has lost four digits.
// Carried directly, g_i = 1 + c'_i obeys
//   s = 1 + A g_(i-1),  g_i = s / (s + C),  -c'_i = C / (s + C),  r'_i = (r_i + A r'_(i-1)) / (s + C)
// with every term non-negative; the back substitution u_i = r'_i + (-c'_i) u_(i+1) has none
// either.  The workspace holds q_i = -c'_i.
struct FgsState {
  float w, g, n, d;  // of the pixel before: its weight to this one, its 1 + c', its two right-hand sides
};

// 1 / x for 1 <= x < 2^100 (here x = s + C >= 1): the hardware reciprocal (1 ulp) and one
// Newton step, three dependent instructions where the IEEE division is a dozen -- the
// division sits on the chain that every step of a line waits for
__device__ __forceinline__ float fgs_rcp(const float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return fmaf(fmaf(-x, r, 1.f), r, r);
}

// returns q = -c' of this pixel; w is its weight to the next one
__device__ __forceinline__ float fgs_eliminate(FgsState& st, const float lam, const float w, const float n,
                                               const float d) {
  const float a = lam * st.w, c = lam * w;
  const float s = 1.f + a * st.g;
  const float inv = fgs_rcp(s + c);
  st.g = s * inv;
  st.n = (n + a * st.n) * inv;
  st.d = (d + a * st.d) * inv;
  st.w = w;
  return c * inv;
}

// ---- the sweep down the first axis of a [B, H, W] plane ----
struct FgsCol {
  float w[kFgsU], n[kFgsU], d[kFgsU], s[kFgsU];
};

// Rows y0 .. y0 + kFgsU - 1 of a column, the row index clamped into the image: every load is
// unconditional and in bounds (a row past the image is loaded twice and never used), so the
// batch is one straight run of loads that the next batch's arithmetic does not wait for.
template <bool FIN>
__device__ __forceinline__ void fgs_col_load(FgsCol& t, const float* pw, const float* pn, const float* pd,
                                             const float* ps, const size_t base, const int y0, const int H,
                                             const int W) {
#pragma unroll
  for (int k = 0; k < kFgsU; ++k) {
    const int y = min(max(y0 + k, 0), H - 1);
    const size_t o = base + (size_t)y * W;
    t.w[k] = pw[o];
    t.n[k] = pn[o];
    t.d[k] = pd[o];
    if (FIN) t.s[k] = ps[o];
  }
}

// FULL: every row of the batch is in the image (no test per row)
template <bool FULL>
__device__ __forceinline__ void fgs_col_forward(const FgsCol& cur, FgsState& st, const float lam, float* cp,
                                                float* num, float* den, const size_t base, const int y0,
                                                const int H, const int W) {
#pragma unroll
  for (int k = 0; k < kFgsU; ++k) {
    const int y = y0 + k;
    if (FULL || y < H) {
      const float q = fgs_eliminate(st, lam, cur.w[k], cur.n[k], cur.d[k]);
      const size_t o = base + (size_t)y * W;
      cp[o] = q;
      num[o] = st.n;
      den[o] = st.d;
    }
  }
}

template <bool FULL, bool FIN>
__device__ __forceinline__ void fgs_col_backward(const FgsCol& cur, float& un, float& ud, float* num, float* den,
                                                 float* refined, float* support, const size_t base, const int y0,
                                                 const int H, const int W) {
#pragma unroll
  for (int k = kFgsU - 1; k >= 0; --k) {
    const int y = y0 + k;
    if (FULL || y < H) {
      un = cur.n[k] + cur.w[k] * un;
      ud = cur.d[k] + cur.w[k] * ud;
      const size_t o = base + (size_t)y * W;
      if (FIN) {
        const float s = cur.s[k];
        refined[o] = ud > kFgsDenMin ? un / ud : (__builtin_isfinite(s) ? s : 0.f);
        if (support) support[o] = ud;
      } else {
        num[o] = un;
        den[o] = ud;
      }
    }
  }
}

// FIN: the last pass of the call: the back substitution divides and writes refined / support
template <bool FIN>
__global__ __launch_bounds__(kWave) void fgs_sweep(const float* __restrict__ wv, float* __restrict__ cp,
                                                      float* __restrict__ num, float* __restrict__ den, int H, int W,
                                                      float lam, const float* __restrict__ disp,
                                                      float* __restrict__ refined, float* __restrict__ support) {
  const int x = blockIdx.x * kWave + threadIdx.x;
  if (x >= W) return;
  const size_t base = (size_t)blockIdx.y * (size_t)H * (size_t)W + x;
  FgsCol cur{}, nxt{};
  FgsState st{0.f, 0.f, 0.f, 0.f};
  fgs_col_load<false>(cur, wv, num, den, nullptr, base, 0, H, W);
  for (int y0 = 0; y0 < H; y0 += kFgsU) {
    fgs_col_load<false>(nxt, wv, num, den, nullptr, base, y0 + kFgsU, H, W);
    if (y0 + kFgsU <= H)
      fgs_col_forward<true>(cur, st, lam, cp, num, den, base, y0, H, W);
    else
      fgs_col_forward<false>(cur, st, lam, cp, num, den, base, y0, H, W);
    cur = nxt;
  }
  // back substitution, the batches in reverse; q of the last row is 0, so it starts itself
  float un = 0.f, ud = 0.f;
  const int ylast = (H - 1) / kFgsU * kFgsU;
  fgs_col_load<FIN>(cur, cp, num, den, disp, base, ylast, H, W);
  for (int y0 = ylast; y0 >= 0; y0 -= kFgsU) {
    fgs_col_load<FIN>(nxt, cp, num, den, disp, base, y0 - kFgsU, H, W);
    if (y0 + kFgsU <= H)
      fgs_col_backward<true, FIN>(cur, un, ud, num, den, refined, support, base, y0, H, W);
    else
      fgs_col_backward<false, FIN>(cur, un, ud, num, den, refined, support, base, y0, H, W);
    cur = nxt;
  }
}

// ---- transposes either side of the horizontal pass ----
// out[b][c][r] = in[b][r][c] for np = 1 or 2 planes per launch (blockIdx.z = np b + plane): a
// 32 x 32 tile goes through LDS, read along c and written along r, 32 lanes on consecutive
// addresses either way.
__global__ __launch_bounds__(kFgsTile * 8) void fgs_transpose(const float* __restrict__ in0, float* __restrict__ out0,
                                                              const float* __restrict__ in1, float* __restrict__ out1,
                                                              int np, int R, int Cn) {
  __shared__ float tile[kFgsTile][kFgsTile + 1];
  const int second = blockIdx.z % np;  // 0 when np = 1: in1 and out1 may then be null
  const float* in = second ? in1 : in0;
  float* out = second ? out1 : out0;
  const size_t base = (size_t)(blockIdx.z / np) * (size_t)R * (size_t)Cn;
  const int tx = threadIdx.x % kFgsTile, ty = threadIdx.x / kFgsTile;
  const int c0 = blockIdx.x * kFgsTile, r0 = blockIdx.y * kFgsTile;
#pragma unroll
  for (int k = 0; k < kFgsTile; k += 8) {
    const int r = r0 + ty + k, c = c0 + tx;
    if (r < R && c < Cn) tile[ty + k][tx] = in[base + (size_t)r * Cn + c];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kFgsTile; k += 8) {
    const int c = c0 + ty + k, r = r0 + tx;
    if (r < R && c < Cn) out[base + (size_t)c * R + r] = tile[tx][ty + k];
  }
}

}  // namespace lea

extern "C" size_t lea_disparity_refine_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * (size_t)H * (size_t)W * lea::kFgsPlanes * sizeof(float);
}

extern "C" int lea_disparity_refine_f32(const float* guide, int64_t guide_bstride, const float* disp,
                                        const float* conf, const uint8_t* exclude, int B, int C, int H, int W,
                                        float lambda, float sigma, int iterations, void* workspace, float* refined,
                                        float* support, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_disparity_refine_f32";
  LEA_CHECK_ARG(guide && disp, "%s: null pointer (guide or disp)", who);
  LEA_CHECK_ARG(workspace, "%s: workspace is null", who);
  LEA_CHECK_ARG(refined, "%s: refined is null", who);
  LEA_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
  LEA_CHECK_ARG(C >= 1 && C <= 4, "%s: C=%d channels (1..4)", who, C);
  LEA_CHECK_ARG(iterations >= 1 && iterations <= 8, "%s: iterations %d (1..8)", who, iterations);
  LEA_CHECK_ARG(lambda > 0.f && lambda <= 3.402823466e+38f, "%s: lambda %g is not a finite number > 0", who,
                (double)lambda);
  LEA_CHECK_ARG(sigma > 0.f && sigma <= 3.402823466e+38f, "%s: sigma %g is not a finite number > 0", who,
                (double)sigma);
  const long long rows = (long long)B * H, hw = (long long)H * W;
  LEA_CHECK_ARG(B <= 32767 && H <= (1 << 21) && W <= (1 << 21) && rows <= 0x7fffffffLL / W,
                "%s: grid too large (B above 32767, H or W above 2^21, or B*H*W above 2^31 - 1)", who);
  LEA_CHECK_ARG(guide_bstride >= (long long)C * hw, "%s: guide batch stride %lld below C*H*W = %lld", who,
                (long long)guide_bstride, (long long)C * hw);
  LEA_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", who);
  const long long n = rows * W;
  {  // no output may overlap an input, the workspace or the other output
    const size_t pn = 4 * (size_t)n;
    const size_t gn = 4 * ((size_t)(B - 1) * (size_t)guide_bstride + (size_t)C * (size_t)hw);
    const void* ins[5] = {guide, disp, conf, exclude, workspace};
    const size_t inn[5] = {gn, pn, pn, (size_t)n, kFgsPlanes * pn};
    const char* inname[5] = {"guide", "disp", "conf", "exclude", "the workspace"};
    const void* outs[2] = {refined, support};
    const char* outname[2] = {"refined", "support"};
    for (int o = 0; o < 2; ++o) {
      if (!outs[o]) continue;
      for (int i = 0; i < 5; ++i)
        LEA_CHECK_ARG(!ins[i] || !spans_overlap(outs[o], pn, ins[i], inn[i]), "%s: %s overlaps %s", who, outname[o],
                      inname[i]);
    }
    LEA_CHECK_ARG(!support || !spans_overlap(refined, pn, support, pn), "%s: refined overlaps support", who);
    for (int i = 0; i < 4; ++i)
      LEA_CHECK_ARG(!ins[i] || !spans_overlap(workspace, kFgsPlanes * pn, ins[i], inn[i]),
                    "%s: the workspace overlaps %s", who, inname[i]);
  }
  float* ws = static_cast<float*>(workspace);
  float *wh = ws, *wv = ws + n, *cp = ws + 2 * n, *num = ws + 3 * n, *den = ws + 4 * n, *wht = ws + 5 * n,
        *dent = ws + 6 * n;
  float* numt = wh;  // free once wh is transposed
  hipStream_t s = as_stream(stream);
  fgs_init<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(guide, guide_bstride, disp, conf, exclude, C, H, W, n, sigma,
                                                      wh, wv, num, den);
  if (int rc = launch_status("lea_disparity_refine_f32 (weights)")) return rc;
  const auto tiles = [](int v) { return (unsigned)((v + kFgsTile - 1) / kFgsTile); };
  const auto lanes = [](int v) { return (unsigned)((v + kWave - 1) / kWave); };
  fgs_transpose<<<dim3(tiles(W), tiles(H), B), kFgsTile * 8, 0, s>>>(wh, wht, nullptr, nullptr, 1, H, W);
  if (int rc = launch_status("lea_disparity_refine_f32 (transpose)")) return rc;
  const double denom = std::pow(4.0, iterations) - 1.0;
  for (int t = 1; t <= iterations; ++t) {
    const float lam = (float)(1.5 * (double)lambda * std::pow(4.0, iterations - t) / denom);
    // horizontal: the rows of [B, H, W] are the lines down the first axis of [B, W, H]
    fgs_transpose<<<dim3(tiles(W), tiles(H), 2 * B), kFgsTile * 8, 0, s>>>(num, numt, den, dent, 2, H, W);
    if (int rc = launch_status("lea_disparity_refine_f32 (transpose)")) return rc;
    fgs_sweep<false><<<dim3(lanes(H), B), kWave, 0, s>>>(wht, cp, numt, dent, W, H, lam, nullptr, nullptr, nullptr);
    if (int rc = launch_status("lea_disparity_refine_f32 (horizontal)")) return rc;
    fgs_transpose<<<dim3(tiles(H), tiles(W), 2 * B), kFgsTile * 8, 0, s>>>(numt, num, dent, den, 2, W, H);
    if (int rc = launch_status("lea_disparity_refine_f32 (transpose)")) return rc;
    if (t < iterations)
      fgs_sweep<false><<<dim3(lanes(W), B), kWave, 0, s>>>(wv, cp, num, den, H, W, lam, nullptr, nullptr, nullptr);
    else
      fgs_sweep<true><<<dim3(lanes(W), B), kWave, 0, s>>>(wv, cp, num, den, H, W, lam, disp, refined, support);
    if (int rc = launch_status("lea_disparity_refine_f32 (vertical)")) return rc;
  }
  return LEA_OK;
}
