// Fused disparity regression: trilinear (align_corners=False) upsample of the
// matching-net output by 3 in D, H, W + softmin over D + sum_d d * p_d.
// Replaces models/build_model_2d.py:52-57 (Disp.forward) and :33-42
// (DisparityRegression.forward).  The [B, maxdisp, 3H3, 3W3] volume the reference
// materialises (425 MB at 576x960 D192 fp32) never exists here.
//
// One thread per output pixel (b, oh, ow), 256 consecutive ow per workgroup.
// The bilinear (h, w) weights and four source columns are fixed per pixel, so the
// thread walks the D axis once: plane values v[dd] = bilerp(cost[dd]) are formed
// on demand (each input plane at most once, d0(od) is monotone), the depth lerp
// gives U[od], and an online softmin (running min m, s = sum e^(m-U), t = sum
// od*e^(m-U), rescaled when m drops) produces disp = t / s.  Reads are the
// 4*D3 cost values per pixel (cache-resident: 3x3 output pixels share them);
// the kernel is bound by the exp/lerp issue, far below HBM time.
#include "disparity_common.h"

namespace lea {

// LDS: the depth axis table (identical for every pixel) and, per thread, one
// batch of bilinearly interpolated cost planes (own column: conflict-free).
template <bool FAST>
__global__ __launch_bounds__(kDispThreads) void disparity_f32(const float* __restrict__ cost,
                                                              float* __restrict__ disp, int D3,
                                                              int H3, int W3, int maxdisp,
                                                              float rd, float rh, float rw) {
#pragma clang fp contract(off)
  extern __shared__ float lds[];
  Axis* tab = reinterpret_cast<Axis*>(lds);                      // [maxdisp]
  float* pv = lds + 4 * maxdisp;                                   // [kDispChunk + 1][threads]
  for (int od = threadIdx.x; od < maxdisp; od += blockDim.x) tab[od] = axis_index(rd, od, D3, maxdisp, 0);
  __syncthreads();
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow = blockIdx.x * blockDim.x + threadIdx.x;
  if (ow >= Wo) return;  // no barrier below
  const int oh = blockIdx.y;
  const int b = blockIdx.z;
  const Axis ah = axis_index(rh, oh, H3, Ho, 0);
  const Axis aw = axis_index(rw, ow, W3, Wo, 0);
  const long long HW = (long long)H3 * W3;
  const float* base = cost + (long long)b * D3 * HW;
  const float* r0 = base + (long long)ah.i0 * W3;
  const float* r1 = base + (long long)ah.i1 * W3;
  float* col = pv + threadIdx.x;

  float m = 0.f, s = 0.f, t = 0.f;
  int od = 0;
  for (int p0 = 0; p0 < D3; p0 += kDispChunk) {
    // planes p0 .. p0 + kDispChunk (one past: the upper lerp source of the last
    // depth in this batch), all loads issued before the first use
#pragma unroll
    for (int k = 0; k <= kDispChunk; ++k) {
      const int dd = min(p0 + k, D3 - 1);
      const long long o = (long long)dd * HW;
      col[k * kDispThreads] = ah.l0 * (aw.l0 * r0[o + aw.i0] + aw.l1 * r0[o + aw.i1]) +
                              ah.l1 * (aw.l0 * r1[o + aw.i0] + aw.l1 * r1[o + aw.i1]);
    }
    for (; od < maxdisp && tab[od].i0 < p0 + kDispChunk; ++od) {
      const Axis ad = tab[od];
      const float u = ad.l0 * col[(ad.i0 - p0) * kDispThreads] + ad.l1 * col[(ad.i1 - p0) * kDispThreads];
      if (od == 0) {
        m = u;
        s = 1.f;
        t = 0.f;
      } else if (u < m) {
        const float f = dexp<FAST>(u - m);  // < 1: rescale what was summed against the old min
        s = s * f + 1.f;
        t = t * f + (float)od;
        m = u;
      } else {
        const float e = dexp<FAST>(m - u);
        s += e;
        t += (float)od * e;
      }
    }
  }
  disp[((long long)b * Ho + oh) * Wo + ow] = t / s;
}

// Register form for the configured depths (r03): D3 and maxdisp compile-time, so the
// thread keeps its D3 bilinearly interpolated plane values v[dd] in registers, the
// depth axis (i0, i1, l0, l1 of every od) folds to constants, and the softmin needs
// no running-minimum rescale: every U[od] is a convex combination of two v's, so
// m = min_dd v[dd] <= min_od U[od] and sum_od e^(m - U) >= e^(m - min U) > 0 -- the same
// ratio t / s as the reference's softmax(-U) (max-subtracted), no divergent branch, no LDS.
template <int D3, int MD, bool FAST>
__global__ __launch_bounds__(kDispThreads) void disparity_reg_f32(const float* __restrict__ cost,
                                                                  float* __restrict__ disp, int H3, int W3,
                                                                  float rh, float rw) {
#pragma clang fp contract(off)
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow = blockIdx.x * blockDim.x + threadIdx.x;
  if (ow >= Wo) return;
  const int oh = blockIdx.y;
  const int b = blockIdx.z;
  const Axis ah = axis_index(rh, oh, H3, Ho, 0);
  const Axis aw = axis_index(rw, ow, W3, Wo, 0);
  const long long HW = (long long)H3 * W3;
  const float* base = cost + (long long)b * D3 * HW;
  const float* r0 = base + (long long)ah.i0 * W3;
  const float* r1 = base + (long long)ah.i1 * W3;
  float v[D3];
#pragma unroll
  for (int dd = 0; dd < D3; ++dd) {
    const long long o = (long long)dd * HW;
    v[dd] = ah.l0 * (aw.l0 * r0[o + aw.i0] + aw.l1 * r0[o + aw.i1]) +
            ah.l1 * (aw.l0 * r1[o + aw.i0] + aw.l1 * r1[o + aw.i1]);
    // 8 planes' loads (32) in flight at a time: issuing all 4 * D3 first took 256 VGPRs
    if (dd % 8 == 7) __builtin_amdgcn_sched_barrier(0);
  }
  float m = v[0];
#pragma unroll
  for (int dd = 1; dd < D3; ++dd) m = fminf(m, v[dd]);
  constexpr float rd = (float)D3 / (float)MD;
  float s = 0.f, t = 0.f;
#pragma unroll
  for (int od = 0; od < MD; ++od) {
    const Axis ad = axis_index(rd, od, D3, MD, 0);  // constants after unrolling
    const float u = ad.l0 * v[ad.i0] + ad.l1 * v[ad.i1];
    const float e = FAST ? dexp<true>(m - u) : exp_noovf(m - u);
    s += e;
    t += (float)od * e;
  }
  disp[((long long)b * Ho + oh) * Wo + ow] = t / s;
}

// Row-staged form (r05; the default for the configured depths): a workgroup owns 256
// consecutive output columns of one output row.  stage_rows2 H-lerps the two source rows its
// pixels read into LDS and each thread forms its planes from there (disp_plane) -- two LDS
// reads per plane instead of four dependent global loads, ~110 fewer VGPRs than the register
// form's load batches (two waves per SIMD there).  The depth axis and softmin are the register
// form's (softmin_twopass), or the factored phase (FACT: softmin_fact).
template <int D3, int MD, bool FAST, bool FACT>
__global__ __launch_bounds__(kDispThreads, 4) void disparity_rows_f32(const float* __restrict__ cost,
                                                                   float* __restrict__ disp, int H3, int W3,
                                                                   float rh, float rw) {
  __shared__ float hl[D3 * kDispCols];
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow0 = blockIdx.x * blockDim.x;
  const int oh = blockIdx.y;
  const int b = blockIdx.z;
  const DispStage st = stage_rows2<D3>(hl, cost, b, oh, ow0, H3, W3, rh, rw);
  __syncthreads();
  const int ow = ow0 + threadIdx.x;
  if (ow >= Wo) return;  // no barrier below
  const DispPlane plane = disp_plane(hl, rw, ow, W3, st.c_lo);
  float r;
  if constexpr (FACT)
    r = softmin_fact<D3, MD, FAST>(plane);
  else
    r = softmin_twopass<FAST>(plane, D3, MD);
  disp[((long long)b * Ho + oh) * Wo + ow] = st.over ? __builtin_nanf("") : r;
}

// Three-row form (r06): one workgroup of 3 x 256 threads owns 256 columns of
// output rows 3k .. 3k + 2.  stage_rows3 loads every raw source value ONCE (three loads per
// staged element, for three H-lerped rows) instead of twice by each of three row workgroups
// (six), and pays the row-position arithmetic once per element; the staged rows, and so every
// output, are bit-identical to disparity_rows_f32's.  LDS 3 * D3 * kDispCols floats (74 KB at
// D3 = 64: two workgroups, 24 waves per CU).
template <int D3, int MD, bool FAST, bool FACT>
__global__ __launch_bounds__(kDisp3Threads) void disparity_rows3_f32(const float* __restrict__ cost,
                                                                   float* __restrict__ disp, int H3, int W3,
                                                                   float rh, float rw) {
  __shared__ float hl[3][D3 * kDispCols];
  const int Ho = 3 * H3, Wo = 3 * W3;
  const int ow0 = blockIdx.x * kDispThreads;
  const int k = blockIdx.y;  // source row k: output rows 3k .. 3k + 2
  const int b = blockIdx.z;
  const DispRows3 st = rows3_span(k, ow0, H3, W3, rh, rw);
  stage_rows3<D3>(hl, cost, b, st, H3, W3);
  __syncthreads();
  const int row = __builtin_amdgcn_readfirstlane(threadIdx.x / kDispThreads);  // wave-uniform
  const int ow = ow0 + (int)threadIdx.x % kDispThreads;
  const int oh = 3 * k + row;
  if (ow >= Wo) return;  // no barrier below
  const DispPlane plane = disp_plane(hl[row], rw, ow, W3, st.c_lo);
  float r;
  if constexpr (FACT)
    r = softmin_fact<D3, MD, FAST>(plane);
  else
    r = softmin_twopass<FAST>(plane, D3, MD);
  disp[((long long)b * Ho + oh) * Wo + ow] = st.over ? __builtin_nanf("") : r;
}

}  // namespace lea

// lea_disparity_set_register_form: 4 (default, r06) = form 3 with D3 exponentials per pixel
// instead of maxdisp (softmin_mean's FACT; the two-row kernel at D3 = 88 likewise), 3 = the three-row staged kernel (C2 69.5 -> 68.3,
// C4 275.6 -> 266.4 us; not at D3 = 88), 2 (r05) = the row-staged kernel for the configured
// (D3, maxdisp), 1 = the register kernel for them, 0 = the online-softmin kernel everywhere
// (A/B and tests)
static LEA_TUNING_INT(lea_disparity_set_register_form, g_disp_reg, 4, 0, 4, "%d")

extern "C" int lea_disparity_regression(const void* cost, float* disp, int B, int D3, int H3,
                                        int W3, int maxdisp, int dtype, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_disparity_regression";
  DispHead h;
  if (int rc = disp_head_check(who, false, nullptr, cost, &disp, 1, B, D3, H3, W3, maxdisp, dtype, &h)) return rc;
  const size_t lds = (size_t)4 * maxdisp * sizeof(float) + (size_t)(kDispChunk + 1) * kDispThreads * sizeof(float);
  LEA_CHECK_ARG(lds <= 65536, "%s: maxdisp %d too large", who, maxdisp);
  const dim3 block(kDispThreads), grid = h.grid;
  const float rh = h.rh, rw = h.rw;
  const bool fast = h.fast, fact = g_disp_reg == 4;
#define LEA_DISP_REG(D3_, MD_)                                                                          \
  if (D3 == D3_ && maxdisp == MD_) {                                                                   \
    auto k_ = fast ? disparity_reg_f32<D3_, MD_, true> : disparity_reg_f32<D3_, MD_, false>;            \
    k_<<<grid, block, 0, as_stream(stream)>>>((const float*)cost, disp, H3, W3, rh, rw);                 \
    return launch_status(who);                                                                         \
  }
  // a staged kernel template's FAST x FACT instantiation for (D3_, MD_), launched if that is the shape
#define LEA_DISP_STAGED(KERNEL, GRID, THREADS, D3_, MD_)                                                \
  if (D3 == D3_ && maxdisp == MD_) {                                                                   \
    auto k_ = fact ? (fast ? KERNEL<D3_, MD_, true, true> : KERNEL<D3_, MD_, false, true>)              \
                   : (fast ? KERNEL<D3_, MD_, true, false> : KERNEL<D3_, MD_, false, false>);           \
    k_<<<GRID, THREADS, 0, as_stream(stream)>>>((const float*)cost, disp, H3, W3, rh, rw);               \
    return launch_status(who);                                                                         \
  }
#define LEA_DISP_ROWS3(D3_, MD_) \
  LEA_DISP_STAGED(disparity_rows3_f32, dim3(grid.x, H3, B), kDisp3Threads, D3_, MD_)
#define LEA_DISP_ROWS(D3_, MD_) LEA_DISP_STAGED(disparity_rows_f32, grid, block, D3_, MD_)
  // (88, 264) -- config 5 -- keeps the two-row kernel: three rows' LDS (101 KB) leave one
  // workgroup per CU there (213 -> 260 us, profiles/r06_disp_probe.txt)
  if (g_disp_reg >= 3 && h.cols_ok) {
    LEA_DISP_ROWS3(4, 12) LEA_DISP_ROWS3(8, 24) LEA_DISP_ROWS3(16, 48) LEA_DISP_ROWS3(32, 96)
    LEA_DISP_ROWS3(64, 192)
  }
  if (g_disp_reg >= 2 && h.cols_ok) {
    LEA_DISP_ROWS(4, 12) LEA_DISP_ROWS(8, 24) LEA_DISP_ROWS(16, 48) LEA_DISP_ROWS(32, 96) LEA_DISP_ROWS(64, 192)
    LEA_DISP_ROWS(88, 264)
  }
#undef LEA_DISP_ROWS
#undef LEA_DISP_ROWS3
#undef LEA_DISP_STAGED
  if (g_disp_reg) {
    // (88, 264) -- config 5 -- stays on the LDS kernel: its 88 plane values take all 256
    // VGPRs, one wave per SIMD (r03: 0.388 vs 0.380 ms); at (64, 192): 0.125 -> 0.081 ms
    LEA_DISP_REG(4, 12) LEA_DISP_REG(8, 24) LEA_DISP_REG(16, 48) LEA_DISP_REG(32, 96) LEA_DISP_REG(64, 192)
  }
#undef LEA_DISP_REG
  auto kern = fast ? disparity_f32<true> : disparity_f32<false>;
  kern<<<grid, block, lds, as_stream(stream)>>>((const float*)cost, disp, D3, H3, W3, maxdisp,
                                               (float)D3 / (float)maxdisp, rh, rw);
  return launch_status(who);
}
