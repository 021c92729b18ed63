// Host-side AddressSanitizer run of the surface model's four entries (lea_dsm_splat_f32,
// lea_dsm_resolve_workspace_bytes, lea_dsm_resolve_f32, lea_dsm_clear), built and run by
// `make asan` after the other drivers, the same way: every csrc unit with ASan on its host
// side, nothing launched.  Each refused call must return LEA_E_INVALID, leave a
// lea_last_error() that names the entry, and touch none of its buffers.
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

static void expect_bytes(const char* what, size_t got, size_t want) {
  if (got != want) {
    std::printf("FAIL workspace bytes %s: %zu (want %zu)\n", what, got, want);
    ++g_fail;
  }
}

// B = 2, rows = 10, a 5 x 6 grid: 60 cells
constexpr int kRows = 20, kCells = 60;
static float pts[3 * kRows], G[24], height[kCells];
static int32_t cnt[2], hits[kCells], source[kCells];
static uint8_t col[3 * kRows], rgb[3 * kCells], state[kCells];
static uint64_t keys[kCells], ws[2 * kCells];

struct Splat {
  const float* p = pts;
  const int32_t* n = cnt;
  const uint8_t* c = col;
  const float* g = G;
  int64_t gs = 12;
  int B = 2, rows = 10, rw = 0;
  float radius = 0.5f;
  int staging = LEA_DSM_STAGING_AUTO, GH = 5, GW = 6;
  uint64_t* k = keys;
  int32_t* h = hits;
};

static int call(const Splat& a) {
  return lea_dsm_splat_f32(a.p, a.n, a.c, a.g, a.gs, a.B, a.rows, a.rw, a.radius, a.staging, a.GH, a.GW, a.k, a.h,
                           nullptr);
}

struct Resolve {
  const uint64_t* k = keys;
  const int32_t* h = hits;
  int B = 2, GH = 5, GW = 6, it = 2, mn = 3;
  float nodata = -1.f;
  void* w = ws;
  float* height = ::height;
  uint8_t* rgb = ::rgb;
  int32_t* source = nullptr;
  uint8_t* state = ::state;
};

static int call(const Resolve& a) {
  return lea_dsm_resolve_f32(a.k, a.h, a.B, a.GH, a.GW, a.it, a.mn, a.nodata, a.w, a.height, a.rgb, a.source, a.state,
                             nullptr);
}

struct Clear {
  uint64_t* k = keys;
  int32_t* h = hits;
  int B = 2, GH = 5, GW = 6;
};

static int call(const Clear& a) { return lea_dsm_clear(a.k, a.h, a.B, a.GH, a.GW, nullptr); }

template <class A, class F>
static void refused(const char* entry, const char* what, F change) {
  A a;
  change(a);
  expect_err(entry, what, call(a), LEA_E_INVALID);
}

int main() {
  if (lea_abi_version() != 14) {
    std::printf("FAIL abi version %d\n", lea_abi_version());
    ++g_fail;
  }
  // two buffers of one uint64 per cell
  expect_bytes("2x5x6", lea_dsm_resolve_workspace_bytes(2, 5, 6), 960);
  expect_bytes("1x1x1", lea_dsm_resolve_workspace_bytes(1, 1, 1), 16);
  expect_bytes("3x2048x2048", lea_dsm_resolve_workspace_bytes(3, 2048, 2048), (size_t)3 * 2048 * 2048 * 16);
  expect_bytes("3x40000x50000", lea_dsm_resolve_workspace_bytes(3, 40000, 50000), (size_t)3 * 2000000000u * 16);
  expect_bytes("B = 0", lea_dsm_resolve_workspace_bytes(0, 5, 6), 0);
  expect_bytes("GH < 0", lea_dsm_resolve_workspace_bytes(2, -5, 6), 0);
  expect_bytes("GW = 0", lea_dsm_resolve_workspace_bytes(2, 5, 0), 0);

  for (float& v : pts) v = -7.f;
  for (float& v : G) v = -7.f;
  for (float& v : height) v = -7.f;
  for (int32_t& v : cnt) v = -7;
  for (int32_t& v : hits) v = -7;
  for (int32_t& v : source) v = -7;
  for (uint8_t& v : col) v = 9;
  for (uint8_t& v : rgb) v = 9;
  for (uint8_t& v : state) v = 9;
  for (uint64_t& v : keys) v = 77;
  for (uint64_t& v : ws) v = 77;
  const float nan = std::nanf("");

  const char* S = "lea_dsm_splat_f32";
  refused<Splat>(S, "null points", [](Splat& a) { a.p = nullptr; });
  refused<Splat>(S, "null G", [](Splat& a) { a.g = nullptr; });
  refused<Splat>(S, "null keys", [](Splat& a) { a.k = nullptr; });
  refused<Splat>(S, "B = 0", [](Splat& a) { a.B = 0; });
  refused<Splat>(S, "B < 0", [](Splat& a) { a.B = -2; });
  refused<Splat>(S, "GH = 0", [](Splat& a) { a.GH = 0; });
  refused<Splat>(S, "GW < 0", [](Splat& a) { a.GW = -6; });
  refused<Splat>(S, "B too large", [](Splat& a) { a.B = 65536, a.GH = 1, a.GW = 1; });
  refused<Splat>(S, "GH*GW = 2^31", [](Splat& a) { a.B = 1, a.GH = 1 << 16, a.GW = 1 << 15; });
  refused<Splat>(S, "GH*GW = 2^40", [](Splat& a) { a.B = 1, a.GH = 1 << 20, a.GW = 1 << 20; });
  refused<Splat>(S, "B*GH*GW = 2^31", [](Splat& a) { a.GH = 1 << 15, a.GW = 1 << 15; });
  refused<Splat>(S, "rows = 0", [](Splat& a) { a.rows = 0; });
  refused<Splat>(S, "rows < 0", [](Splat& a) { a.rows = -10; });
  refused<Splat>(S, "B*rows = 2^31", [](Splat& a) { a.rows = 1 << 30; });
  refused<Splat>(S, "row_width < 0", [](Splat& a) { a.rw = -1; });
  refused<Splat>(S, "row_width above rows", [](Splat& a) { a.rw = 11; });
  refused<Splat>(S, "G stride 8", [](Splat& a) { a.gs = 8; });
  refused<Splat>(S, "G stride < 0", [](Splat& a) { a.gs = -12; });
  refused<Splat>(S, "radius < 0", [](Splat& a) { a.radius = -0.5f; });
  refused<Splat>(S, "radius above the limit", [](Splat& a) { a.radius = 2.5f; });
  refused<Splat>(S, "radius NaN", [nan](Splat& a) { a.radius = nan; });
  refused<Splat>(S, "radius inf", [](Splat& a) { a.radius = INFINITY; });
  refused<Splat>(S, "staging 3", [](Splat& a) { a.staging = 3; });
  refused<Splat>(S, "staging -1", [](Splat& a) { a.staging = -1; });
  refused<Splat>(S, "misaligned keys", [](Splat& a) { a.k = (uint64_t*)((char*)keys + 4); });
  refused<Splat>(S, "misaligned points", [](Splat& a) { a.p = (const float*)((const char*)pts + 2); });
  refused<Splat>(S, "misaligned G", [](Splat& a) { a.g = (const float*)((const char*)G + 1); });
  refused<Splat>(S, "misaligned count", [](Splat& a) { a.n = (const int32_t*)((const char*)cnt + 2); });
  refused<Splat>(S, "misaligned hits", [](Splat& a) { a.h = (int32_t*)((char*)hits + 2); });
  refused<Splat>(S, "keys = points", [](Splat& a) { a.k = (uint64_t*)pts; });
  refused<Splat>(S, "keys = G", [](Splat& a) { a.B = 1, a.GH = 1, a.GW = 1, a.k = (uint64_t*)G; });
  refused<Splat>(S, "keys in the second matrix", [](Splat& a) { a.GH = 1, a.GW = 1, a.k = (uint64_t*)(G + 22); });
  refused<Splat>(S, "keys = count", [](Splat& a) { a.GH = 1, a.GW = 1, a.k = (uint64_t*)cnt; });
  refused<Splat>(S, "hits = colours", [](Splat& a) { a.GH = 1, a.GW = 1, a.h = (int32_t*)col; });
  refused<Splat>(S, "hits in points' last float", [](Splat& a) { a.h = (int32_t*)(pts + 3 * kRows - 1); });
  refused<Splat>(S, "hits = keys", [](Splat& a) { a.h = (int32_t*)keys; });
  refused<Splat>(S, "hits in keys' last word", [](Splat& a) { a.h = (int32_t*)(keys + kCells) - 1; });
  // the optional ones may be null: the next check in line fires
  refused<Splat>(S, "null count, colours and hits, then staging", [](Splat& a) {
    a.n = nullptr, a.c = nullptr, a.h = nullptr, a.staging = 7;
  });
  // with one matrix for all (stride 0) only its 12 floats are G: keys behind them is no overlap
  refused<Splat>(S, "G stride 0, keys behind the matrix, then hits", [](Splat& a) {
    a.gs = 0, a.GH = 1, a.GW = 1, a.k = (uint64_t*)(G + 12), a.h = (int32_t*)(G + 13);
  });

  const char* R = "lea_dsm_resolve_f32";
  refused<Resolve>(R, "null keys", [](Resolve& a) { a.k = nullptr; });
  refused<Resolve>(R, "every output null", [](Resolve& a) {
    a.height = nullptr, a.rgb = nullptr, a.source = nullptr, a.state = nullptr;
  });
  refused<Resolve>(R, "rgb and source", [](Resolve& a) { a.source = source; });
  refused<Resolve>(R, "B = 0", [](Resolve& a) { a.B = 0; });
  refused<Resolve>(R, "GH < 0", [](Resolve& a) { a.GH = -5; });
  refused<Resolve>(R, "GW = 0", [](Resolve& a) { a.GW = 0; });
  refused<Resolve>(R, "B too large", [](Resolve& a) { a.B = 65536, a.GH = 1, a.GW = 1; });
  refused<Resolve>(R, "B*GH*GW = 2^31", [](Resolve& a) { a.GH = 1 << 15, a.GW = 1 << 15; });
  refused<Resolve>(R, "iterations < 0", [](Resolve& a) { a.it = -1; });
  refused<Resolve>(R, "iterations above the limit", [](Resolve& a) { a.it = 1025; });
  refused<Resolve>(R, "min_neighbours 0", [](Resolve& a) { a.mn = 0; });
  refused<Resolve>(R, "min_neighbours 9", [](Resolve& a) { a.mn = 9; });
  refused<Resolve>(R, "null workspace with passes", [](Resolve& a) { a.w = nullptr; });
  refused<Resolve>(R, "misaligned keys", [](Resolve& a) { a.k = (const uint64_t*)((const char*)keys + 4); });
  refused<Resolve>(R, "misaligned workspace", [](Resolve& a) { a.w = (char*)ws + 4; });
  refused<Resolve>(R, "misaligned height", [](Resolve& a) { a.height = (float*)((char*)height + 2); });
  refused<Resolve>(R, "misaligned source", [](Resolve& a) {
    a.rgb = nullptr, a.source = (int32_t*)((char*)source + 1);
  });
  refused<Resolve>(R, "misaligned hits", [](Resolve& a) { a.h = (const int32_t*)((const char*)hits + 2); });
  refused<Resolve>(R, "height = keys", [](Resolve& a) { a.height = (float*)keys; });
  refused<Resolve>(R, "state in keys' last byte", [](Resolve& a) { a.state = (uint8_t*)(keys + kCells) - 1; });
  refused<Resolve>(R, "source = hits", [](Resolve& a) { a.rgb = nullptr, a.source = hits; });
  refused<Resolve>(R, "rgb in the workspace", [](Resolve& a) { a.rgb = (uint8_t*)(ws + kCells); });
  refused<Resolve>(R, "height in the workspace's last word", [](Resolve& a) {
    a.height = (float*)(ws + 2 * kCells) - 1;
  });
  refused<Resolve>(R, "state = rgb", [](Resolve& a) { a.state = rgb; });
  refused<Resolve>(R, "state in height's last byte", [](Resolve& a) { a.state = (uint8_t*)(height + kCells) - 1; });
  refused<Resolve>(R, "workspace = keys", [](Resolve& a) { a.w = keys; });
  refused<Resolve>(R, "workspace = hits", [](Resolve& a) { a.B = 1, a.GH = 1, a.GW = 1, a.w = hits; });
  // without passes the workspace may be null: the next check in line fires
  refused<Resolve>(R, "no passes, null workspace and hits, then an overlap", [](Resolve& a) {
    a.it = 0, a.w = nullptr, a.h = nullptr, a.state = (uint8_t*)height;
  });

  const char* C = "lea_dsm_clear";
  refused<Clear>(C, "null keys", [](Clear& a) { a.k = nullptr; });
  refused<Clear>(C, "B = 0", [](Clear& a) { a.B = 0; });
  refused<Clear>(C, "GH = 0", [](Clear& a) { a.GH = 0; });
  refused<Clear>(C, "GW < 0", [](Clear& a) { a.GW = -1; });
  refused<Clear>(C, "B too large", [](Clear& a) { a.B = 65536, a.GH = 1, a.GW = 1; });
  refused<Clear>(C, "B*GH*GW = 2^31", [](Clear& a) { a.GH = 1 << 15, a.GW = 1 << 15; });
  refused<Clear>(C, "misaligned keys", [](Clear& a) { a.k = (uint64_t*)((char*)keys + 4); });
  refused<Clear>(C, "misaligned hits", [](Clear& a) { a.h = (int32_t*)((char*)hits + 2); });
  refused<Clear>(C, "hits = keys", [](Clear& a) { a.h = (int32_t*)keys; });
  refused<Clear>(C, "null hits, then the shape", [](Clear& a) { a.h = nullptr, a.GW = 0; });

  bool wrote = false;
  for (float v : pts) wrote |= v != -7.f;
  for (float v : G) wrote |= v != -7.f;
  for (float v : height) wrote |= v != -7.f;
  for (int32_t v : cnt) wrote |= v != -7;
  for (int32_t v : hits) wrote |= v != -7;
  for (int32_t v : source) wrote |= v != -7;
  for (uint8_t v : col) wrote |= v != 9;
  for (uint8_t v : rgb) wrote |= v != 9;
  for (uint8_t v : state) wrote |= v != 9;
  for (uint64_t v : keys) wrote |= v != 77;
  for (uint64_t v : ws) wrote |= v != 77;
  if (wrote) {
    std::printf("FAIL a refused call wrote to a buffer\n");
    ++g_fail;
  }
  if (g_fail)
    std::printf("FAIL dsm: %d failed checks\n", g_fail);
  else
    std::printf("OK: 0 failed checks\n");
  return g_fail ? 1 : 0;
}
