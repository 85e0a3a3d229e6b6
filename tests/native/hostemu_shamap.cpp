// hostemu_shamap.cpp -- TEST HARNESS ONLY.  Compiles the SHAMap root's shared
// device code (stellard_amd/csrc/stl_shamap_core.h) for the host: the nibble,
// the common prefix, the node rule and the inner-node hash one by one, and the
// whole root as the kernels of stl_shamap.hip compute it, step by step on
// exactly sized heap arrays (a stable sort by the core's key order stands in
// for the radix passes).  Not part of the product library.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../stellard_amd/csrc/stl_shamap_core.h"

namespace {
void load(uint32_t w[8], const uint8_t* p) { stl::shamap_load_key(w, p, 0); }
}  // namespace

extern "C" {

uint32_t hostemu_shamap_nibble(const uint8_t key[32], uint32_t d) {
  uint32_t w[8];
  load(w, key);
  const uint32_t a = stl::shamap_nibble(w, d), b = stl::shamap_nibble_bytes(key, d);
  return a == b ? a : 0xFFFFFFFFu;  // the two forms agree
}

uint32_t hostemu_shamap_common_prefix(const uint8_t a[32], const uint8_t b[32]) {
  uint32_t x[8], y[8];
  load(x, a);
  load(y, b);
  return stl::shamap_common_prefix(x, y);
}

int hostemu_shamap_key_less(const uint8_t a[32], const uint8_t b[32]) {
  uint32_t x[8], y[8];
  load(x, a);
  load(y, b);
  return stl::shamap_key_less(x, y) ? 1 : 0;
}

uint64_t hostemu_shamap_sort_word(const uint8_t key[32], uint32_t w) {
  uint32_t x[8];
  load(x, key);
  return stl::shamap_sort_word(x, w);
}

int32_t hostemu_shamap_neighbour(const uint8_t key[32], const uint8_t next[32], int last, int only) {
  uint32_t x[8], y[8] = {};
  load(x, key);
  if (next) load(y, next);
  return stl::shamap_neighbour(x, y, last != 0, only != 0);
}

int hostemu_shamap_starts_node(int32_t l_prev, int32_t l_cur, int32_t d) {
  return stl::shamap_starts_node(l_prev, l_cur, d) ? 1 : 0;
}

int32_t hostemu_shamap_leaf_parent_depth(int32_t l_prev, int32_t l_cur) {
  return stl::shamap_leaf_parent_depth(l_prev, l_cur);
}

// slots: 16 * 32 bytes -> out: 32 bytes
void hostemu_shamap_inner_hash(const uint8_t* slots, uint8_t out[32]) {
  std::vector<uint32_t> rec(stl::kShamapRecordWords);
  rec[0] = stl::kShamapInnerPrefix;
  std::memcpy(rec.data() + 1, slots, 512);
  uint32_t h[8];
  stl::shamap_inner_hash(h, rec.data());
  std::memcpy(out, h, 32);
}

uint32_t hostemu_shamap_range_end(const uint8_t* skey, uint32_t m, uint32_t a, uint32_t d) {
  return stl::shamap_range_end(skey, m, a, d);
}

uint32_t hostemu_shamap_branch_first(const uint8_t* skey, uint32_t a, uint32_t e, uint32_t d, uint32_t c) {
  return stl::shamap_branch_first(skey, a, e, d, c);
}

// The whole computation as stl_shamap.hip stages it.  key, leaf (nullable):
// n * 32 bytes; select (nullable): ceil(n / 8) bytes; root: 32 bytes; counts: 4
// words; hist (nullable): 64 words, the inner nodes per depth; l_out
// (nullable): counts[0] neighbour bytes.  Returns 0, or -1 when an invariant
// of the level step fails (more than 128 nodes in 256 positions).
int hostemu_shamap_root(const uint8_t* key, const uint8_t* leaf, const uint8_t* select, uint32_t n, uint8_t* root,
                        uint32_t* counts, uint32_t* hist_out, int8_t* l_out) {
  auto selected = [&](uint32_t r) { return !select || ((select[r >> 3] >> (r & 7u)) & 1u); };
  // 1. sort: the selected rows by key, stably, then the others
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
    uint32_t x[8], y[8];
    load(x, key + 32 * (size_t)a);
    load(y, key + 32 * (size_t)b);
    return stl::shamap_key_less(x, y);
  });
  std::stable_partition(perm.begin(), perm.end(), selected);
  // 2. heads and the compaction
  std::vector<uint8_t> skey, slot;
  uint32_t nsel = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!selected(perm[i])) continue;
    ++nsel;
    if (i > 0) {
      uint32_t x[8], y[8];
      load(x, key + 32 * (size_t)perm[i]);
      load(y, key + 32 * (size_t)perm[i - 1]);
      if (stl::shamap_common_prefix(x, y) == 64u) continue;
    }
    const uint8_t* k = key + 32 * (size_t)perm[i];
    const uint8_t* h = leaf ? leaf + 32 * (size_t)perm[i] : k;
    skey.insert(skey.end(), k, k + 32);
    slot.insert(slot.end(), h, h + 32);
  }
  const uint32_t m = (uint32_t)(skey.size() / 32);
  // 3. neighbours
  std::vector<int8_t> l(m);
  uint32_t hist[stl::kShamapDepths] = {};
  for (uint32_t j = 0; j < m; ++j) {
    uint32_t a[8], b[8] = {};
    load(a, skey.data() + 32 * (size_t)j);
    int32_t lp = -1;
    if (j > 0) {
      load(b, skey.data() + 32 * (size_t)(j - 1));
      lp = (int32_t)stl::shamap_common_prefix(b, a);
    }
    const bool last = j + 1 == m;
    if (!last) load(b, skey.data() + 32 * (size_t)(j + 1));
    const int32_t lc = stl::shamap_neighbour(a, b, last, m == 1);
    l[j] = (int8_t)lc;
    for (int32_t d = lp + 1; d <= lc; ++d) ++hist[d];
  }
  // 4. levels: chunks of 256 positions, every record of a chunk gathered before any slot is
  // written (the kernel hashes several chunks' nodes together; the order of reads and writes
  // within a group is this one)
  for (int32_t d = (int32_t)stl::kShamapDepths - 1; d >= 0; --d) {
    if (!hist[d]) continue;
    for (uint32_t t0 = 0; t0 < m; t0 += 256) {
      std::vector<uint32_t> pos;
      for (uint32_t i = t0; i < m && i < t0 + 256; ++i)
        if (stl::shamap_starts_node(i ? (int32_t)l[i - 1] : -1, (int32_t)l[i], d)) pos.push_back(i);
      if (pos.size() > 128) return -1;
      std::vector<uint32_t> rec(pos.size() * stl::kShamapRecordWords, 0u);
      for (size_t k = 0; k < pos.size(); ++k) {
        const uint32_t a = pos[k], e = stl::shamap_range_end(skey.data(), m, a, (uint32_t)d);
        uint32_t* r = rec.data() + k * stl::kShamapRecordWords;
        r[0] = stl::kShamapInnerPrefix;
        for (uint32_t c = 0; c < stl::kShamapBranches; ++c) {
          const uint32_t p = stl::shamap_branch_first(skey.data(), a, e, (uint32_t)d, c);
          if (p < e) std::memcpy(r + 1 + 8 * c, slot.data() + 32 * (size_t)p, 32);
        }
      }
      for (size_t k = 0; k < pos.size(); ++k) {
        uint32_t h[8];
        stl::shamap_inner_hash(h, rec.data() + k * stl::kShamapRecordWords);
        std::memcpy(slot.data() + 32 * (size_t)pos[k], h, 32);
      }
    }
  }
  // 5. finish
  std::memset(root, 0, 32);
  if (m) std::memcpy(root, slot.data(), 32);
  uint32_t sum = 0, deep = 0;
  for (uint32_t d = 0; d < stl::kShamapDepths; ++d) {
    sum += hist[d];
    if (hist[d]) deep = d;
  }
  if (counts) {
    counts[0] = m;
    counts[1] = nsel - m;
    counts[2] = sum;
    counts[3] = deep;
  }
  if (hist_out) std::memcpy(hist_out, hist, sizeof(hist));
  if (l_out && m) std::memcpy(l_out, l.data(), m);
  return 0;
}

}  // extern "C"
