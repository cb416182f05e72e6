// Stress driver for the block manager's prefix index (run under ASan+UBSan / TSan by
// tests/test_kv_prefix_sanitizers.py).  4 threads publish, match, reserve and release against one
// small pool, so evictions happen all the time; the manager's self-check runs throughout.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

extern "C" {
void* lumen_kv_create(int);
void lumen_kv_destroy(void*);
int lumen_kv_free_blocks(void*);
int lumen_kv_cached_blocks(void*);
int lumen_kv_num_seqs(void*);
int lumen_kv_reserve(void*, int64_t, int);
int lumen_kv_can_reserve(void*, int64_t, int);
int lumen_kv_table(void*, int64_t, int*, int);
int lumen_kv_release(void*, int64_t);
int lumen_kv_publish(void*, int64_t, const uint64_t*, int);
int lumen_kv_match(void*, const uint64_t*, int, int64_t);
int lumen_kv_check(void*);
}

namespace {
constexpr int kBlocks = 48, kThreads = 4, kIters = 4000, kPrompts = 12, kMaxDepth = 6;

// prompt p, block i: chained keys shared by every thread (the same prompts come back again and again)
void keys_of(int p, int n, uint64_t* out) {
  for (int i = 0; i < n; ++i) {
    out[2 * i] = 0x9e3779b97f4a7c15ull * (uint64_t)(p * 64 + i + 1);
    out[2 * i + 1] = 0xc2b2ae3d27d4eb4full ^ (uint64_t)(p * 1000003 + i);
  }
}
}  // namespace

int main() {
  void* h = lumen_kv_create(kBlocks);
  std::atomic<int> bad{0}, hits{0}, published{0}, denied{0};
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      std::mt19937 rng(1234 + t);
      uint64_t keys[2 * kMaxDepth];
      int tab[16];
      for (int it = 0; it < kIters && !bad.load(); ++it) {
        const int64_t seq = (int64_t)t * 1000000 + it + 1;
        const int p = (int)(rng() % kPrompts);
        const int depth = 1 + (int)(rng() % kMaxDepth);             // full blocks of the prompt
        const int tokens = depth * 64 + (int)(rng() % 64) + 1;      // plus a partial one
        keys_of(p, depth, keys);
        const int got = lumen_kv_match(h, keys, depth, seq);
        if (got < 0 || got % 64 != 0 || got > depth * 64) bad = 10;
        if (got > 0) ++hits;
        if (lumen_kv_reserve(h, seq, tokens) < 0) {
          ++denied;
          if (got > 0) lumen_kv_release(h, seq);
          continue;
        }
        const int nb = lumen_kv_table(h, seq, tab, 16);
        if (nb != depth + 1) bad = 11;
        for (int i = 0; i < nb && i < 16; ++i)
          if (tab[i] < 0 || tab[i] >= kBlocks) bad = 12;
        if (rng() % 4 != 0) {
          const int add = lumen_kv_publish(h, seq, keys, depth);
          if (add < 0) bad = 13;
          published += add > 0 ? add : 0;
        }
        if (lumen_kv_publish(h, seq, keys, depth + 2) != -1) bad = 14;   // more than its full blocks
        const int free_now = lumen_kv_free_blocks(h), idle_now = lumen_kv_cached_blocks(h);
        if (free_now < 0 || free_now > kBlocks || idle_now < 0 || idle_now > kBlocks) bad = 15;
        if (it % 16 == 0) {
          const int c = lumen_kv_check(h);
          if (c) bad = 100 + c;
        }
        if (lumen_kv_release(h, seq) != 0) bad = 16;
      }
    });
  for (auto& x : th) x.join();
  int c = lumen_kv_check(h);
  if (c) bad = 100 + c;
  if (lumen_kv_num_seqs(h) != 0 || lumen_kv_free_blocks(h) != kBlocks) bad = 17;
  // whatever is left is index-only: one big reservation evicts all of it
  const int idle = lumen_kv_cached_blocks(h);
  if (lumen_kv_reserve(h, 1, kBlocks * 64) != kBlocks || lumen_kv_cached_blocks(h) != 0) bad = 18;
  c = lumen_kv_check(h);
  if (c) bad = 100 + c;
  lumen_kv_release(h, 1);
  if (lumen_kv_free_blocks(h) != kBlocks || lumen_kv_check(h)) bad = 19;
  lumen_kv_destroy(h);
  if (bad.load() || hits.load() == 0 || published.load() == 0) {
    std::printf("FAIL code=%d hits=%d published=%d denied=%d\n", bad.load(), hits.load(), published.load(), denied.load());
    return 1;
  }
  std::printf("ok hits=%d published=%d denied=%d idle_at_end=%d\n", hits.load(), published.load(), denied.load(), idle);
  return 0;
}
