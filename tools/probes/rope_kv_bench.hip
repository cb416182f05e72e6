// RoPE + KV-write kernel timing without torch: the plain forms (tile kernel at a prefill's row count,
// per-element kernel at a decode batch's) and the multimodal-RoPE forms (contiguous and interleaved
// axis layout) of csrc/llm.hip, device events around windows of launches replayed from a graph (so
// the host's enqueue rate does not bound the short kernels), the variants' windows interleaved.  Linked against csrc/llm.hip directly, so two checkouts' kernels can be timed by two
// binaries run in turn on one box (-DNO_MROPE: a checkout whose RopeKVArgs has no mrope fields).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Ilumen_amd/csrc tools/probes/rope_kv_bench.hip \
//         lumen_amd/csrc/llm.hip -o rope_kv_bench && ./rope_kv_bench [windows] [launches per window]
// The launches of a window rotate the same rows in place (a rotation keeps their magnitude) and
// write the same cache slots: 7.7 MB of QKV rows, so the numbers are cache-warm kernel times.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "llm.h"

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP %s @%d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

static uint16_t bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return (uint16_t)((u + 0x7fff + ((u >> 16) & 1)) >> 16);
}

template <class T>
static T* upload(const std::vector<T>& h) {
  T* d;
  CHECK(hipMalloc(&d, h.size() * sizeof(T)));
  CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

#ifndef NO_MROPE
// two-bit axis codes of frequency 0 .. 63 (D = 128), sections (t, h, w)
static void axis_codes(const int sec[3], bool interleaved, uint64_t out[2]) {
  out[0] = out[1] = 0;
  for (int i = 0; i < 64; ++i) {
    uint64_t ax;
    if (interleaved) ax = (i % 3 == 1 && i < 3 * sec[1]) ? 1 : (i % 3 == 2 && i < 3 * sec[2]) ? 2 : 0;
    else ax = (i >= sec[0]) + (i >= sec[0] + sec[1]);
    out[i >> 5] |= ax << ((i & 31) * 2);
  }
}
#endif

int main(int argc, char** argv) {
  const int windows = argc > 1 ? atoi(argv[1]) : 15, per = argc > 2 ? atoi(argv[2]) : 200;
  const int H = 32, Hkv = 8, D = 128, HALF = D / 2, MAXPOS = 8192;
  const int T_TILE = 624, T_ELEM = 16;                  // a 576-token image + 48 text tokens; a decode batch
  const int64_t ld = (int64_t)(H + 2 * Hkv) * D;
  const int NB = (T_TILE + 63) / 64;

  std::vector<uint16_t> qkv((size_t)T_TILE * ld);
  uint32_t r = 12345;
  for (auto& v : qkv) {
    r = r * 1664525u + 1013904223u;
    v = bf16(((r >> 8) & 0xffff) / 32768.f - 1.f);
  }
  std::vector<float> cs((size_t)MAXPOS * HALF * 2);
  for (int p = 0; p < MAXPOS; ++p)
    for (int i = 0; i < HALF; ++i) {
      const double a = p * std::pow(1e6, -2.0 * i / D);
      cs[((size_t)p * HALF + i) * 2] = (float)std::cos(a);
      cs[((size_t)p * HALF + i) * 2 + 1] = (float)std::sin(a);
    }
  // three-axis positions: 24 text tokens, a 24 x 24 image grid, 24 text tokens; the plain forms get
  // the cache indices, as a 1-D decoder does
  std::vector<int> pos(T_TILE), pos3(3 * (size_t)T_TILE);
  std::vector<int64_t> slots(T_TILE);
  int n = 0;
  for (int t = 0; t < T_TILE; ++t) {
    pos[t] = t;
    slots[t] = t;
    const int c = t - 24;
    if (c >= 0 && c < 576) {
      pos3[t] = n; pos3[T_TILE + t] = n + c / 24; pos3[2 * T_TILE + t] = n + c % 24;
      if (c == 575) n += 24;
    } else {
      pos3[t] = pos3[T_TILE + t] = pos3[2 * T_TILE + t] = n++;
    }
  }
  // the per-element launch reads its own [3, T_ELEM] array: rows are T apart
  std::vector<int> pos3e(3 * (size_t)T_ELEM);
  for (int a = 0; a < 3; ++a)
    for (int t = 0; t < T_ELEM; ++t) pos3e[a * T_ELEM + t] = pos3[(size_t)a * T_TILE + 20 + t];

  lumen::RopeKVArgs base{};
  base.qkv = upload(qkv); base.ld = ld;
  base.cos_sin = upload(cs);
  base.slots = upload(slots);
  CHECK(hipMalloc(&base.k_cache, (size_t)NB * Hkv * 64 * D * 2));
  CHECK(hipMalloc(&base.v_cache, (size_t)NB * Hkv * 64 * D * 2));
  base.H = H; base.Hkv = Hkv; base.D = D;
  const int* d_pos = upload(pos);

  struct Variant { std::string name; lumen::RopeKVArgs a; std::vector<float> us; hipGraphExec_t g; };
  std::vector<Variant> vs;
  auto add = [&](const char* name, int T, const int* p, int mrope, const int* sec, bool inter) {
    lumen::RopeKVArgs a = base;
    a.T = T; a.pos = p;
#ifndef NO_MROPE
    a.mrope = mrope;
    if (mrope) axis_codes(sec, inter, a.mrope_axes);
#endif
    vs.push_back({name, a, {}, nullptr});
  };
  add("tile T=624 plain", T_TILE, d_pos, 0, nullptr, false);
  add("elem T=16  plain", T_ELEM, d_pos, 0, nullptr, false);
#ifndef NO_MROPE
  const int sec2[3] = {16, 24, 24}, sec3[3] = {24, 20, 20};
  const int* d_pos3 = upload(pos3);
  const int* d_pos3e = upload(pos3e);
  add("tile T=624 mrope contiguous [16,24,24]", T_TILE, d_pos3, 1, sec2, false);
  add("tile T=624 mrope interleaved [24,20,20]", T_TILE, d_pos3, 1, sec3, true);
  add("elem T=16  mrope interleaved [24,20,20]", T_ELEM, d_pos3e, 1, sec3, true);
#endif

  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (auto& v : vs)                                   // warm-up: code objects, caches
    for (int i = 0; i < 20; ++i) CHECK(lumen::rope_kv(v.a, st));
  CHECK(hipStreamSynchronize(st));
  for (auto& v : vs) {                                 // one window = one graph of `per` serial launches
    hipGraph_t g;
    CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < per; ++i) CHECK(lumen::rope_kv(v.a, st));
    CHECK(hipStreamEndCapture(st, &g));
    CHECK(hipGraphInstantiate(&v.g, g, nullptr, nullptr, 0));
    CHECK(hipGraphLaunch(v.g, st));
    CHECK(hipStreamSynchronize(st));
  }
  for (int w = 0; w < windows; ++w)
    for (auto& v : vs) {
      CHECK(hipEventRecord(e0, st));
      CHECK(hipGraphLaunch(v.g, st));
      CHECK(hipEventRecord(e1, st));
      CHECK(hipEventSynchronize(e1));
      float ms;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      v.us.push_back(ms * 1000.f / per);
    }
  for (auto& v : vs) {
    std::sort(v.us.begin(), v.us.end());
    printf("%-42s median %7.2f us  (min %7.2f  max %7.2f; %d windows x %d launches)\n", v.name.c_str(),
           v.us[v.us.size() / 2], v.us.front(), v.us.back(), windows, per);
  }
  return 0;
}
