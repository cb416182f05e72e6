// Paged-KV block manager (host runtime, C ABI for ctypes).
//
// The VLM engine keeps every sequence's KV in 64-token blocks of one large
// per-layer pool on the GPU (layouts in ../llm.h).  This manager owns the
// block free list, per-sequence block tables and reference counts (prefix
// sharing between sequences forked from a common prompt); the Python engine
// asks it for capacity before each step and copies the tables it returns
// into the device block-table tensor.  Thread-safe (one mutex): the engine
// thread allocates while request threads may query stats.
//
// Prefix index: a finished prompt publishes its full blocks under 128-bit
// chained content keys; the index holds one reference per block, so the
// block outlives its sequence.  A later prompt matches the longest leading
// run of its keys and starts from those blocks.  A block held by the index
// alone ("idle") counts as free: reserve evicts idle blocks when the free
// list runs short, least recently matched first and, within one chain (same
// match), deepest first.  A block any live sequence holds is never evicted.
#include <algorithm>
#include <cstdint>
#include <mutex>
#include <set>
#include <tuple>
#include <unordered_map>
#include <vector>

namespace {

constexpr int kBlock = 64;

struct Seq {
  std::vector<int> blocks;
  int tokens = 0;
};

struct Key {
  uint64_t a, b;
  bool operator==(const Key& o) const { return a == o.a && b == o.b; }
};
struct KeyHash {
  size_t operator()(const Key& k) const { return (size_t)(k.a ^ (k.b * 0x9e3779b97f4a7c15ull)); }
};

// what the index knows about a published block
struct Cached {
  Key key{0, 0};
  uint64_t tick = 0;   // last publish / match (LRU clock)
  int depth = 0;       // position in its prompt's chain
  bool in = false;     // the index holds a reference to this block
};

struct Manager {
  explicit Manager(int n) : ref(n, 0), cached(n) {
    free.reserve(n);
    for (int i = n - 1; i >= 0; --i) free.push_back(i);
  }
  std::mutex mu;
  std::vector<int> free;
  std::vector<int> ref;            // live sequences holding the block + 1 if the index does
  std::unordered_map<int64_t, Seq> seqs;
  std::unordered_map<Key, int, KeyHash> index;        // content key -> block
  std::vector<Cached> cached;
  std::set<std::tuple<uint64_t, int, int>> idle;      // (tick, -depth, block) of index-only blocks: eviction order
  uint64_t clock = 0;

  std::tuple<uint64_t, int, int> order(int b) const { return {cached[b].tick, -cached[b].depth, b}; }
  int available() const { return (int)free.size() + (int)idle.size(); }

  // n blocks on the free list, evicting idle blocks if needed (caller checked available())
  void make_free(int n) {
    while ((int)free.size() < n) {
      const int b = std::get<2>(*idle.begin());
      idle.erase(idle.begin());
      index.erase(cached[b].key);
      cached[b].in = false;
      ref[b] = 0;
      free.push_back(b);
    }
  }
  int take() {
    const int b = free.back();
    free.pop_back();
    ref[b] = 1;
    return b;
  }
  void share(int b) {   // one more sequence holds b
    if (cached[b].in && ref[b] == 1) idle.erase(order(b));
    ++ref[b];
  }
  void drop(int b) {
    if (--ref[b] == 0) free.push_back(b);
    else if (ref[b] == 1 && cached[b].in) idle.insert(order(b));
  }
};

}  // namespace

extern "C" {

void* lumen_kv_create(int num_blocks) { return num_blocks > 0 ? new Manager(num_blocks) : nullptr; }

void lumen_kv_destroy(void* h) { delete static_cast<Manager*>(h); }

int lumen_kv_free_blocks(void* h) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  return m->available();   // index-only blocks are handed out on demand
}

// Blocks held by the prefix index alone (reusable by a match, evictable by a reserve).
int lumen_kv_cached_blocks(void* h) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  return (int)m->idle.size();
}

int lumen_kv_num_seqs(void* h) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  return (int)m->seqs.size();
}

// Grow sequence `seq` to hold `n_tokens` tokens.  Returns the number of blocks the
// sequence now owns, or -1 (and changes nothing) when the pool cannot supply them.
int lumen_kv_reserve(void* h, int64_t seq, int n_tokens) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  Seq& s = m->seqs[seq];
  const int need = (n_tokens + kBlock - 1) / kBlock - (int)s.blocks.size();
  if (need > m->available()) {
    if (s.blocks.empty()) m->seqs.erase(seq);
    return -1;
  }
  m->make_free(need);
  for (int i = 0; i < need; ++i) s.blocks.push_back(m->take());
  s.tokens = std::max(s.tokens, n_tokens);
  return (int)s.blocks.size();
}

// Would reserving n_tokens for `seq` succeed?  (admission control)
int lumen_kv_can_reserve(void* h, int64_t seq, int n_tokens) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  auto it = m->seqs.find(seq);
  const int have = it == m->seqs.end() ? 0 : (int)it->second.blocks.size();
  return (n_tokens + kBlock - 1) / kBlock - have <= m->available();
}

// Copy up to `max` block ids of `seq` into `out`; returns the block count (-1: unknown seq).
int lumen_kv_table(void* h, int64_t seq, int* out, int max) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  auto it = m->seqs.find(seq);
  if (it == m->seqs.end()) return -1;
  const auto& b = it->second.blocks;
  const int n = std::min<int>((int)b.size(), max);
  std::copy(b.begin(), b.begin() + n, out);
  return (int)b.size();
}

// Share the full blocks of `src` with a new sequence `dst` (prefix caching).  The
// partially filled last block is NOT shared: the caller re-computes / copies it.
// Returns the number of tokens covered by the shared blocks, or -1.
int lumen_kv_fork(void* h, int64_t src, int64_t dst) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  auto it = m->seqs.find(src);
  if (it == m->seqs.end() || m->seqs.count(dst)) return -1;
  const int full = it->second.tokens / kBlock;
  Seq d;
  for (int i = 0; i < full; ++i) {
    const int b = it->second.blocks[i];
    m->share(b);
    d.blocks.push_back(b);
  }
  d.tokens = full * kBlock;
  m->seqs[dst] = d;
  return d.tokens;
}

// Register the first n blocks of `seq` (all full) under keys[2i], keys[2i + 1].  The index takes
// one reference per newly registered block; a key already present keeps its existing block.
// Returns the number of blocks newly registered, or -1 (unknown seq / more blocks than it holds).
int lumen_kv_publish(void* h, int64_t seq, const uint64_t* keys, int n) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  auto it = m->seqs.find(seq);
  if (it == m->seqs.end() || n < 0 || n > (int)it->second.blocks.size() || n > it->second.tokens / kBlock) return -1;
  const uint64_t tick = ++m->clock;
  int added = 0;
  for (int i = 0; i < n; ++i) {
    const Key k{keys[2 * i], keys[2 * i + 1]};
    const int b = it->second.blocks[i];
    if (m->cached[b].in || !m->index.emplace(k, b).second) continue;   // block or key already published
    m->cached[b] = Cached{k, tick, i, true};
    ++m->ref[b];   // held by seq as well: not idle
    ++added;
  }
  return added;
}

// Longest leading run of keys present in the index -> new sequence `dst` sharing those blocks.
// Returns the tokens covered (0: nothing matched, no sequence created; -1: dst exists).
int lumen_kv_match(void* h, const uint64_t* keys, int n, int64_t dst) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  if (m->seqs.count(dst)) return -1;
  Seq d;
  for (int i = 0; i < n; ++i) {
    auto it = m->index.find(Key{keys[2 * i], keys[2 * i + 1]});
    if (it == m->index.end()) break;
    d.blocks.push_back(it->second);
  }
  if (d.blocks.empty()) return 0;
  const uint64_t tick = ++m->clock;
  for (int b : d.blocks) {
    m->share(b);                 // leaves the idle set under its old tick
    m->cached[b].tick = tick;
  }
  d.tokens = (int)d.blocks.size() * kBlock;
  const int tokens = d.tokens;
  m->seqs[dst] = std::move(d);
  return tokens;
}

// Self-check of the bookkeeping (tests): 0 when every reference count equals the number of
// sequences holding the block plus the index's reference, no block on the free list is referenced
// or indexed, every block is either free or referenced, and the idle set is exactly the
// index-only blocks; otherwise a positive code naming the broken invariant.
int lumen_kv_check(void* h) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  const int n = (int)m->ref.size();
  std::vector<int> want(n, 0), on_free(n, 0);
  for (const auto& kv : m->seqs)
    for (int b : kv.second.blocks) {
      if (b < 0 || b >= n) return 1;
      ++want[b];
    }
  for (const auto& kv : m->index) {
    const int b = kv.second;
    if (b < 0 || b >= n || !m->cached[b].in || !(m->cached[b].key == kv.first)) return 2;
    ++want[b];
  }
  int indexed = 0;
  for (int b = 0; b < n; ++b) indexed += m->cached[b].in ? 1 : 0;
  if (indexed != (int)m->index.size()) return 3;
  for (int b : m->free) {
    if (b < 0 || b >= n || on_free[b]++) return 4;
    if (m->ref[b] != 0 || m->cached[b].in) return 5;
  }
  size_t idle = 0;
  for (int b = 0; b < n; ++b) {
    if (m->ref[b] != want[b]) return 6;
    if ((m->ref[b] == 0) != (on_free[b] == 1)) return 7;
    if (m->cached[b].in && m->ref[b] == 1) {
      ++idle;
      if (!m->idle.count(m->order(b))) return 8;
    }
  }
  return idle == m->idle.size() ? 0 : 9;
}

int lumen_kv_release(void* h, int64_t seq) {
  auto* m = static_cast<Manager*>(h);
  std::lock_guard<std::mutex> g(m->mu);
  auto it = m->seqs.find(seq);
  if (it == m->seqs.end()) return -1;
  for (int b : it->second.blocks) m->drop(b);
  m->seqs.erase(it);
  return 0;
}

}  // extern "C"
