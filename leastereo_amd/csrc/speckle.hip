// Speckle filter of a disparity map: connected-component labelling (4-neighbours, two pixels
// connected when neither is a wall and |a - b| <= max_diff) and the removal of the components
// of at most max_size pixels (OpenCV's filterSpeckles).  The definition is at
// lea_disparity_speckle_f32 in include/leastereo_hip.h.
//
// Four launches on one stream, ordered by the launch boundaries and by nothing else:
//   1. speckle_local    a workgroup labels a 64 x 16 tile in LDS: a wave owns a row, so the
//                       horizontal runs come from one ballot of the right-connectivity bits
//                       and only the vertical links go through the union-find (LDS atomicMin).
//                       It writes every pixel's parent as the image index of its tile-local
//                       root, and at each local root the pixel count of the local component.
//   2. speckle_merge    one lane per connected pixel pair across a tile seam: union of the two
//                       roots in global memory (atomicMin).
//   3. speckle_flatten  every local root walks to its root, stores it as its parent and, if it
//                       is not the root itself, adds its local count to the root's counter,
//                       through an LDS table that sums what a 64 x 64 strip sends to one root.
//   4. speckle_apply    a pixel's root is its parent's parent; labels, size, state, filtered.
//
// No lane ever waits for a value another lane has yet to write: there is no lock, no spin and
// no barrier between workgroups.  Every loop walks a strictly decreasing label: a parent is
// never above its child (parent[i] <= i holds from the first store on and atomicMin keeps it),
// so find() ends at a root after at most i steps, and union() retries only when its atomicMin
// returned a value below the root it meant to link, i.e. with a strictly smaller pair.  The
// links go from the larger root to the smaller, so the root of a finished component is its
// smallest index: the labels do not depend on scheduling; the counts are integer sums.
// Integer atomics only; no host copy, no allocation.
#include <cmath>

#include "common.h"

namespace lea {

constexpr int kSpTW = 64;                       // tile width: one wave per row
constexpr int kSpTH = 16;                       // tile height
constexpr int kSpPix = kSpTW * kSpTH;           // pixels of a tile
constexpr int kSpThreads = 256;                 // 4 waves, each owns kSpRows consecutive rows
constexpr int kSpRows = kSpTH / (kSpThreads / kWave);
constexpr int kSpStrip = 64;                    // rows of a flatten strip (four tiles)
constexpr int kSpSlotBits = 10;
constexpr int kSpSlots = 1 << kSpSlotBits;      // LDS table of a flatten strip: root -> summed count
constexpr int kSpProbes = 16;                   // slots tried before the add goes to memory directly
constexpr int kSpeckleState = LEA_LR_SPECKLE;

static_assert(kSpTW == kWave, "a wave owns a tile row");

// a and b are connected values (walls are NaN here, or tested by the caller): the subtraction
// is exactly rounded, NaN and an overflow to inf compare false
__device__ __forceinline__ bool sp_conn(const float a, const float b, const float max_diff) {
  return fabsf(a - b) <= max_diff;
}

// ---- union-find on the LDS labels of a tile ----
// lab[x] <= x always, so the walk strictly decreases until lab[x] == x
__device__ __forceinline__ int sp_find_lds(int* lab, int x) {
  for (;;) {
    const int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}

// every retry continues with old < b in place of b and find(a) <= a: a + b strictly decreases
__device__ __forceinline__ void sp_union_lds(int* lab, int a, int b) {
  for (;;) {
    a = sp_find_lds(lab, a);
    b = sp_find_lds(lab, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&lab[b], a);
    if (old == b) return;
    b = old;
  }
}

// ---- union-find on the parents in global memory, while other workgroups rewrite them ----
__device__ __forceinline__ int sp_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[x] <= x always (never negative for a pixel that is not a wall): strictly decreasing
__device__ __forceinline__ int sp_find(const int* parent, int x) {
  for (;;) {
    const int p = sp_load(&parent[x]);
    if (p == x) return x;
    x = p;
  }
}

// as sp_union_lds; a read that is behind the memory only lengthens the walk, since every value
// a parent ever held is an ancestor, and the atomicMin's return is what decides
__device__ __forceinline__ void sp_union(int* parent, int a, int b) {
  for (;;) {
    a = sp_find(parent, a);
    b = sp_find(parent, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&parent[b], a);
    if (old == b) return;
    b = old;
  }
}

// Stage 1.  LDS: val, lab, cnt are rows of 64 dwords, a wave reads or writes one row (or the
// row below) per instruction: lane x is on bank x mod 32 in each half-wave, no conflict; the
// atomics land where the data sends them.  bits holds a byte per pixel, four lanes to a dword
// (a broadcast).  13 KiB a workgroup.
__global__ __launch_bounds__(kSpThreads) void speckle_local(const float* __restrict__ disp,
                                                            const unsigned char* __restrict__ exclude, int H, int W,
                                                            float max_diff, int* __restrict__ parent,
                                                            int* __restrict__ count) {
  __shared__ float val[kSpPix];
  __shared__ int lab[kSpPix];
  __shared__ int cnt[kSpPix];
  __shared__ unsigned char bits[kSpPix];  // 1: connected to the right, 2: connected down
  const int lx = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int x0 = blockIdx.x * kSpTW, y0 = blockIdx.y * kSpTH;
  const size_t base = (size_t)blockIdx.z * (size_t)H * (size_t)W;
  const int gx = x0 + lx;
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int k = 0; k < kSpRows; ++k) {
    const int ly = wave * kSpRows + k, gy = y0 + ly;
    float v = nan;  // a wall, or outside the image
    if (gx < W && gy < H) {
      const size_t o = base + (size_t)gy * W + gx;
      const float d = disp[o];
      if (__builtin_isfinite(d) && !(exclude && exclude[o])) v = d;
    }
    val[ly * kSpTW + lx] = v;
    cnt[ly * kSpTW + lx] = 0;
  }
  __syncthreads();
  int start[kSpRows], len[kSpRows];
#pragma unroll
  for (int k = 0; k < kSpRows; ++k) {
    const int ly = wave * kSpRows + k, p = ly * kSpTW + lx;
    const float v = val[p];
    const bool right = lx < kSpTW - 1 && sp_conn(v, val[lx < kSpTW - 1 ? p + 1 : p], max_diff);
    const bool down = ly < kSpTH - 1 && sp_conn(v, val[ly < kSpTH - 1 ? p + kSpTW : p], max_diff);
    // the row's runs: bit x of brk = no link between x and x + 1 (bit 63 always)
    const unsigned long long brk = ~__ballot(right);
    const unsigned long long below = brk & ((1ull << lx) - 1ull);
    start[k] = below ? 64 - __builtin_clzll(below) : 0;
    len[k] = __builtin_ctzll(brk >> lx) + 1;
    lab[p] = ly * kSpTW + start[k];
    bits[p] = (unsigned char)((right ? 1 : 0) | (down ? 2 : 0));
  }
  __syncthreads();
  // vertical links; one is skipped when the pixel to the left makes the same one (it is linked
  // to this pixel, to the one below itself, and that one to the one below this)
#pragma unroll
  for (int k = 0; k < kSpRows; ++k) {
    const int ly = wave * kSpRows + k, p = ly * kSpTW + lx;
    if (bits[p] & 2) {
      const bool same = lx > 0 && (bits[p - 1] & 3) == 3 && (bits[p + kSpTW - 1] & 1);
      if (!same) sp_union_lds(lab, p, p + kSpTW);
    }
  }
  __syncthreads();
  int root[kSpRows];
#pragma unroll
  for (int k = 0; k < kSpRows; ++k) {
    const int ly = wave * kSpRows + k, p = ly * kSpTW + lx;
    root[k] = sp_find_lds(lab, p);
    // one add per run, by its first pixel (a wall is a run of its own and counts nothing)
    if (start[k] == lx && val[p] == val[p]) atomicAdd(&cnt[root[k]], len[k]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSpRows; ++k) {
    const int ly = wave * kSpRows + k, gy = y0 + ly, p = ly * kSpTW + lx;
    if (gx < W && gy < H) {
      const size_t o = base + (size_t)gy * W + gx;
      const bool wall = !(val[p] == val[p]);
      const int r = root[k];
      parent[o] = wall ? -1 : (y0 + r / kSpTW) * W + x0 + r % kSpTW;
      count[o] = (!wall && r == p) ? cnt[p] : 0;
    }
  }
}

// Stage 2.  Lanes 0 .. nh*W - 1 take the pairs across the horizontal seams (below rows 15, 31,
// ...), the rest the pairs across the vertical seams (right of columns 63, 127, ...).  A lane
// whose pair joins the same two parents as its neighbour lane's is skipped.
__global__ __launch_bounds__(kSpThreads) void speckle_merge(const float* __restrict__ disp, int H, int W, int nh,
                                                            int nv, float max_diff, int* __restrict__ parent) {
  const size_t base = (size_t)blockIdx.y * (size_t)H * (size_t)W;
  const long long t = (long long)blockIdx.x * kSpThreads + threadIdx.x;
  const long long th = (long long)nh * W, total = th + (long long)nv * H;
  int a = -1, b = -1;  // the pair, as image indices
  if (t < th) {
    const int y = (int)(t / W) * kSpTH + kSpTH - 1, x = (int)(t % W);
    a = y * W + x;
    b = a + W;
  } else if (t < total) {
    const long long u = t - th;
    // down a seam, so that neighbour lanes join one tile pair
    const int y = (int)(u % H), x = (int)(u / H) * kSpTW + kSpTW - 1;
    a = y * W + x;
    b = a + 1;
  }
  int pa = -1, pb = -1;
  if (a >= 0) {
    pa = sp_load(&parent[base + a]);
    pb = sp_load(&parent[base + b]);
    if (pa < 0 || pb < 0 || !sp_conn(disp[base + a], disp[base + b], max_diff)) pa = pb = -1;
  }
  const int qa = __shfl_up(pa, 1), qb = __shfl_up(pb, 1);
  const bool same = (threadIdx.x & (kWave - 1)) != 0 && qa == pa && qb == pb;
  if (pa >= 0 && !same) sp_union(parent + base, pa, pb);
}

// Stage 3, the work of the local roots alone (count > 0 marks them; the seams rewrote no other
// pixel's parent): each walks to its root, stores it as its parent and adds its local count to
// the root's counter.  The parents are rewritten while others walk them (to the root, a smaller
// ancestor), so loads and stores of them are agent-scope atomics here too.  count[] of a pixel
// that is not the root of its component is written by nobody in this launch; a root reads its
// own, whatever has been added to it, and does nothing.
// A workgroup takes a strip of 64 x 64 pixels (four tiles, a wave per row) and sums the counts
// that go to one root in an LDS table first (open addressing: a slot is claimed by atomicCAS,
// at most kSpProbes slots are tried, then the add goes to global memory directly -- nobody
// waits for a slot), so a component that fills the image costs one global add per strip on
// its one counter, not one per tile-local component: those serialise at the memory.
__global__ __launch_bounds__(kSpThreads) void speckle_flatten(int H, int W, int* __restrict__ parent,
                                                              int* __restrict__ count) {
  __shared__ int key[kSpSlots];
  __shared__ int sum[kSpSlots];
  for (int s = threadIdx.x; s < kSpSlots; s += kSpThreads) {
    key[s] = -1;
    sum[s] = 0;
  }
  __syncthreads();
  const size_t base = (size_t)blockIdx.z * (size_t)H * (size_t)W;
  int* par = parent + base;
  int* cnt = count + base;
  const int x = blockIdx.x * kSpTW + (threadIdx.x & (kWave - 1));
  const int y0 = blockIdx.y * kSpStrip + threadIdx.x / kWave;  // this wave's rows: y0, y0 + 4, ...
  constexpr int kWaves = kSpThreads / kWave, kMine = kSpStrip / kWaves;
  int mine[kMine];  // all of this lane's counts in flight at once; 0 outside the image
#pragma unroll
  for (int k = 0; k < kMine; ++k) {
    const int y = y0 + k * kWaves;
    mine[k] = (x < W && y < H) ? cnt[y * W + x] : 0;
  }
#pragma unroll
  for (int k = 0; k < kMine; ++k) {
    const int c = mine[k];
    if (c <= 0) continue;
    const int i = (y0 + k * kWaves) * W + x;
    const int g = sp_find(par, i);
    if (g == i) continue;
    __hip_atomic_store(&par[i], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned h = ((unsigned)g * 2654435761u) >> (32 - kSpSlotBits);
    bool placed = false;
    for (int t = 0; t < kSpProbes && !placed; ++t) {
      const int old = atomicCAS(&key[h], -1, g);
      if (old == -1 || old == g) {
        atomicAdd(&sum[h], c);
        placed = true;
      }
      h = (h + 1) & (kSpSlots - 1);
    }
    if (!placed) atomicAdd(&cnt[g], c);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kSpSlots; s += kSpThreads)
    if (key[s] >= 0) atomicAdd(&cnt[key[s]], sum[s]);
}

// Stage 4.  A pixel's parent is its local root (or, for a local root, the root), whose parent
// is the root since stage 3: two loads.
__global__ __launch_bounds__(kSpThreads) void speckle_apply(const float* __restrict__ disp,
                                                            const unsigned char* __restrict__ exclude, int hw,
                                                            int max_size, float fill, const int* __restrict__ parent,
                                                            const int* __restrict__ count, int* __restrict__ labels,
                                                            int* __restrict__ size, unsigned char* __restrict__ state,
                                                            float* __restrict__ filtered) {
  const long long i = (long long)blockIdx.x * kSpThreads + threadIdx.x;
  if (i >= hw) return;
  const size_t base = (size_t)blockIdx.y * (size_t)hw, o = base + i;
  const int lr = parent[o];
  const int p = lr < 0 ? -1 : parent[base + lr];
  const int n = p < 0 ? 0 : count[base + p];
  if (labels) labels[o] = p;
  if (size) size[o] = n;
  if (state || filtered) {
    const unsigned char e = exclude ? exclude[o] : 0;
    // a wall without an exclude flag is a non-finite disparity: no evidence
    const unsigned char s = e ? e : (unsigned char)((p < 0 || n <= max_size) ? kSpeckleState : 0);
    if (state) state[o] = s;
    if (filtered) filtered[o] = s ? fill : disp[o];
  }
}

}  // namespace lea

extern "C" size_t lea_disparity_speckle_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * (size_t)H * (size_t)W * 2 * sizeof(int);
}

extern "C" int lea_disparity_speckle_f32(const float* disp, const uint8_t* exclude, int B, int H, int W,
                                         float max_diff, int max_size, float fill, void* workspace, int32_t* labels,
                                         int32_t* size, uint8_t* state, float* filtered, void* stream) {
  using namespace lea;
  clear_error();
  const char* who = "lea_disparity_speckle_f32";
  LEA_CHECK_ARG(disp, "%s: disp is null", who);
  LEA_CHECK_ARG(workspace, "%s: workspace is null", who);
  LEA_CHECK_ARG(labels || size || state || filtered, "%s: every output is null", who);
  LEA_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
  LEA_CHECK_ARG(B <= 65535, "%s: B=%d above 65535", who, B);
  LEA_CHECK_ARG((long long)H * W <= 0x7fffffffLL, "%s: H*W = %lld is not below 2^31", who, (long long)H * W);
  LEA_CHECK_ARG(max_diff >= 0.f && max_diff <= 3.402823466e+38f, "%s: max_diff %g is not a finite number >= 0", who,
                (double)max_diff);
  LEA_CHECK_ARG(max_size >= 0, "%s: max_size %d is negative", who, max_size);
  LEA_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", who);
  const int hw = H * W;
  const size_t n = (size_t)B * (size_t)hw;
  {  // no output may overlap an input, the workspace or another output
    const void* ins[3] = {disp, exclude, workspace};
    const size_t inn[3] = {4 * n, n, 8 * n};
    const char* inname[3] = {"disp", "exclude", "the workspace"};
    const void* outs[4] = {labels, size, state, filtered};
    const size_t outn[4] = {4 * n, 4 * n, n, 4 * n};
    const char* outname[4] = {"labels", "size", "state", "filtered"};
    for (int o = 0; o < 4; ++o) {
      if (!outs[o]) continue;
      for (int i = 0; i < 3; ++i)
        LEA_CHECK_ARG(!ins[i] || !spans_overlap(outs[o], outn[o], ins[i], inn[i]), "%s: %s overlaps %s", who,
                      outname[o], inname[i]);
      for (int q = 0; q < o; ++q)
        LEA_CHECK_ARG(!outs[q] || !spans_overlap(outs[o], outn[o], outs[q], outn[q]), "%s: %s overlaps %s", who,
                      outname[o], outname[q]);
    }
    for (int i = 0; i < 2; ++i)
      LEA_CHECK_ARG(!ins[i] || !spans_overlap(workspace, 8 * n, ins[i], inn[i]), "%s: the workspace overlaps %s", who,
                    inname[i]);
  }
  int* parent = static_cast<int*>(workspace);
  int* count = parent + n;
  hipStream_t s = as_stream(stream);
  const unsigned tx = (unsigned)((W + kSpTW - 1) / kSpTW), ty = (unsigned)((H + kSpTH - 1) / kSpTH);
  LEA_CHECK_ARG(ty <= 65535, "%s: H=%d above %d", who, H, 65535 * kSpTH);
  speckle_local<<<dim3(tx, ty, (unsigned)B), kSpThreads, 0, s>>>(disp, exclude, H, W, max_diff, parent, count);
  if (int rc = launch_status("lea_disparity_speckle_f32 (tiles)")) return rc;
  const int nh = (H - 1) / kSpTH, nv = (W - 1) / kSpTW;  // seams
  const long long pairs = (long long)nh * W + (long long)nv * H;
  if (pairs > 0) {
    speckle_merge<<<dim3((unsigned)((pairs + kSpThreads - 1) / kSpThreads), (unsigned)B), kSpThreads, 0, s>>>(
        disp, H, W, nh, nv, max_diff, parent);
    if (int rc = launch_status("lea_disparity_speckle_f32 (seams)")) return rc;
  }
  const dim3 flat((unsigned)(((long long)hw + kSpThreads - 1) / kSpThreads), (unsigned)B);
  const dim3 strips(tx, (unsigned)((H + kSpStrip - 1) / kSpStrip), (unsigned)B);
  speckle_flatten<<<strips, kSpThreads, 0, s>>>(H, W, parent, count);
  if (int rc = launch_status("lea_disparity_speckle_f32 (flatten)")) return rc;
  speckle_apply<<<flat, kSpThreads, 0, s>>>(disp, exclude, hw, max_size, fill, parent, count, labels, size, state,
                                            filtered);
  return launch_status("lea_disparity_speckle_f32 (apply)");
}
