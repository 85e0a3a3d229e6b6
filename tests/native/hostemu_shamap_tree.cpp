// hostemu_shamap_tree.cpp -- TEST HARNESS ONLY.  Compiles the resident SHAMap's
// shared device code (stellard_amd/csrc/stl_shamap_tree_core.h) for the host:
// the rules one by one, and a whole apply as the kernels of stl_shamap_tree.hip
// stage it, step by step on exactly sized heap arrays (a stable sort by the
// core's key order stands in for the radix passes, running sums for the
// scans).  Not part of the product library.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../stellard_amd/csrc/stl_shamap_tree_core.h"

namespace {

void load(uint32_t w[8], const uint8_t* p) { stl::shamap_load_key(w, p, 0); }

struct Gen {
  std::vector<uint8_t> key, leaf;    // capacity * 32 each
  std::vector<uint32_t> bcnt, bh;    // 65,536 and 65,536 * 8
  uint32_t count = 0;
  uint32_t root[8] = {};
};

struct Tree {
  uint32_t cap = 0;
  int live = 0;
  Gen g[2];
};

// Depths 63 down to d_last over m sorted keys with their slots, as the level
// kernel does: chunks of 256 positions, a chunk's records gathered before any
// slot is written.  False when a chunk lists more than 128 nodes.
bool levels(const std::vector<uint8_t>& skey, std::vector<uint8_t>& slot, uint32_t m, uint32_t d_last) {
  std::vector<int8_t> l(m ? m : 1);
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
  for (int32_t d = (int32_t)stl::kShamapDepths - 1; d >= (int32_t)d_last; --d) {
    if (!hist[d]) continue;
    for (uint32_t t0 = 0; t0 < m; t0 += 256) {
      std::vector<uint32_t> pos;
      for (uint32_t i = t0; i < m && i < t0 + 256; ++i)
        if (stl::shamap_starts_node(i ? (int32_t)l[i - 1] : -1, (int32_t)l[i], d)) pos.push_back(i);
      if (pos.size() > 128) return false;
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
  return true;
}

}  // namespace

extern "C" {

uint32_t hostemu_tree_bucket(const uint8_t key[32]) {
  uint32_t w[8];
  load(w, key);
  return stl::shamap_tree_bucket(w);
}

int hostemu_tree_head(int is_last, uint32_t cp_next) { return stl::shamap_tree_head(is_last != 0, cp_next) ? 1 : 0; }

int32_t hostemu_tree_delta(int is_delete, int found) { return stl::shamap_tree_delta(is_delete != 0, found != 0); }

uint32_t hostemu_tree_item_dest(uint32_t i, uint32_t before) { return stl::shamap_tree_item_dest(i, before); }

uint32_t hostemu_tree_insert_dest(uint32_t pos, uint32_t before) { return stl::shamap_tree_insert_dest(pos, before); }

uint32_t hostemu_tree_changes_before(const uint32_t* pos, const uint8_t* code, uint32_t k, uint32_t i, int* hit) {
  bool h = false;
  const uint32_t r = stl::shamap_tree_changes_before(pos, code, k, i, &h);
  *hit = h ? 1 : 0;
  return r;
}

uint32_t hostemu_tree_lower_bound(const uint8_t* skey, uint32_t m, const uint8_t key[32], int* found) {
  uint32_t w[8];
  load(w, key);
  bool f = false;
  const uint32_t p = stl::shamap_tree_lower_bound(skey, m, w, &f);
  *found = f ? 1 : 0;
  return p;
}

uint32_t hostemu_tree_bucket_begin(const uint8_t* skey, uint32_t m, uint32_t b) {
  return stl::shamap_tree_bucket_begin(skey, m, b);
}

// cnt: 16 words; h: 16 * 32 bytes; out: 32 bytes -> the count
uint32_t hostemu_tree_top_value(const uint32_t* cnt, const uint8_t* h, int root, uint8_t out[32]) {
  std::vector<uint32_t> hw(128);
  std::memcpy(hw.data(), h, 512);
  uint32_t o[8];
  const uint32_t c = stl::shamap_tree_top_value(cnt, hw.data(), root != 0, o);
  std::memcpy(out, o, 32);
  return c;
}

void* hostemu_tree_new(uint32_t cap) {
  Tree* t = new Tree();
  t->cap = cap;
  for (Gen& g : t->g) {
    g.key.assign(32 * (size_t)cap, 0);
    g.leaf.assign(32 * (size_t)cap, 0);
    g.bcnt.assign(stl::kTreeBuckets, 0);
    g.bh.assign(8 * (size_t)stl::kTreeBuckets, 0);
  }
  return t;
}

void hostemu_tree_free(void* h) { delete static_cast<Tree*>(h); }

// key / leaf: capacity * 32 bytes -> the live generation's sorted content; returns the count.
uint32_t hostemu_tree_export(void* h, uint8_t* key, uint8_t* leaf) {
  const Tree* t = static_cast<Tree*>(h);
  const Gen& g = t->g[t->live];
  std::memcpy(key, g.key.data(), 32 * (size_t)g.count);
  std::memcpy(leaf, g.leaf.data(), 32 * (size_t)g.count);
  return g.count;
}

// One apply as stl_shamap_tree.hip stages it.  key, leaf (nullable), op
// (nullable): the batch of n rows; root: 32 bytes; counts: 8 words.  Returns 0;
// -1 when the count after the batch would exceed the capacity (nothing changes:
// only work arrays have been written by then); -2 when an
// invariant fails (a destination past the capacity or past the new count, more
// than 128 nodes in 256 positions): the tree is then unchanged as well -- only
// the other generation has been written.
int hostemu_tree_apply(void* h, const uint8_t* key, const uint8_t* leaf, const uint8_t* op, uint32_t n, uint8_t* root,
                       uint32_t* counts) {
  Tree* t = static_cast<Tree*>(h);
  const Gen& from = t->g[t->live];
  Gen& to = t->g[t->live ^ 1];
  const uint32_t cap = t->cap, m = from.count;
  if (n == 0) {
    std::memcpy(root, from.root, 32);
    if (counts) {
      std::memset(counts, 0, 32);
      counts[0] = m;
    }
    return 0;
  }
  // 1. changes: stable sort, the last of equal keys, compaction
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
    uint32_t x[8], y[8];
    load(x, key + 32 * (size_t)a);
    load(y, key + 32 * (size_t)b);
    return stl::shamap_key_less(x, y);
  });
  std::vector<uint8_t> ckey, cleaf, code;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t cp = 0;
    if (i + 1 < n) {
      uint32_t x[8], y[8];
      load(x, key + 32 * (size_t)perm[i]);
      load(y, key + 32 * (size_t)perm[i + 1]);
      cp = stl::shamap_common_prefix(x, y);
    }
    if (!stl::shamap_tree_head(i + 1 == n, cp)) continue;
    const uint32_t row = perm[i];
    const bool del = op && op[row] != 0;
    const uint8_t* k = key + 32 * (size_t)row;
    const uint8_t* lh = (leaf && !del) ? leaf + 32 * (size_t)row : k;
    ckey.insert(ckey.end(), k, k + 32);
    cleaf.insert(cleaf.end(), lh, lh + 32);
    code.push_back(del ? (uint8_t)stl::kTreeOpDelete : (uint8_t)0);
  }
  const uint32_t k = (uint32_t)code.size();
  // 2. locate, the scan, the dirty buckets
  std::vector<uint32_t> pos(k), delta(k), scan(k);
  std::vector<uint32_t> dirty(stl::kTreeBuckets, 0u);
  uint32_t ins = 0, rep = 0, dele = 0, absent = 0;
  for (uint32_t j = 0; j < k; ++j) {
    uint32_t w[8];
    load(w, ckey.data() + 32 * (size_t)j);
    bool found = false;
    pos[j] = stl::shamap_tree_lower_bound(from.key.data(), m, w, &found);
    const bool is_del = (code[j] & stl::kTreeOpDelete) != 0;
    delta[j] = (uint32_t)stl::shamap_tree_delta(is_del, found);
    code[j] = (uint8_t)((is_del ? stl::kTreeOpDelete : 0u) | (found ? stl::kTreeFound : 0u));
    dirty[stl::shamap_tree_bucket(w)] = 1u;
    ins += !is_del && !found;
    rep += !is_del && found;
    dele += is_del && found;
    absent += is_del && !found;
  }
  uint32_t run = 0;
  for (uint32_t j = 0; j < k; ++j) {
    scan[j] = run;
    run += delta[j];
  }
  const uint32_t total = ins - dele, m2 = m + total;
  if (run != total) return -2;
  if (m2 > cap) return -1;
  // 3. merge into the other generation; every row of it below m2 must be written exactly once
  std::vector<uint8_t> written(m2 ? m2 : 1, 0);
  for (uint32_t i = 0; i < m; ++i) {
    bool hit = false;
    const uint32_t r = stl::shamap_tree_changes_before(pos.data(), code.data(), k, i, &hit);
    if (hit && (code[r] & stl::kTreeOpDelete)) continue;
    const uint32_t dst = stl::shamap_tree_item_dest(i, r < k ? scan[r] : total);
    if (dst >= m2 || written[dst]++) return -2;
    std::memcpy(to.key.data() + 32 * (size_t)dst, from.key.data() + 32 * (size_t)i, 32);
    std::memcpy(to.leaf.data() + 32 * (size_t)dst,
                hit ? cleaf.data() + 32 * (size_t)r : from.leaf.data() + 32 * (size_t)i, 32);
  }
  for (uint32_t j = 0; j < k; ++j) {
    if (code[j] & (stl::kTreeOpDelete | stl::kTreeFound)) continue;
    const uint32_t dst = stl::shamap_tree_insert_dest(pos[j], scan[j]);
    if (dst >= m2 || written[dst]++) return -2;
    std::memcpy(to.key.data() + 32 * (size_t)dst, ckey.data() + 32 * (size_t)j, 32);
    std::memcpy(to.leaf.data() + 32 * (size_t)dst, cleaf.data() + 32 * (size_t)j, 32);
  }
  for (uint32_t i = 0; i < m2; ++i)
    if (!written[i]) return -2;
  // 4. bucket bounds
  std::vector<uint32_t> lb(stl::kTreeBuckets + 1);
  for (uint32_t b = 0; b <= stl::kTreeBuckets; ++b) lb[b] = stl::shamap_tree_bucket_begin(to.key.data(), m2, b);
  // 5. the dirty buckets' subtrees in a scratch of their own
  std::vector<uint32_t> sz(stl::kTreeBuckets), off(stl::kTreeBuckets);
  uint32_t gathered = 0, ndirty = 0;
  for (uint32_t b = 0; b < stl::kTreeBuckets; ++b) {
    sz[b] = dirty[b] ? lb[b + 1] - lb[b] : 0u;
    off[b] = gathered;
    gathered += sz[b];
    ndirty += dirty[b];
  }
  std::vector<uint8_t> skey(32 * (size_t)gathered), slot(32 * (size_t)gathered);
  for (uint32_t p = 0; p < gathered; ++p) {
    const uint32_t b = (uint32_t)(std::upper_bound(off.begin(), off.end(), p) - off.begin()) - 1;
    const uint32_t src = lb[b] + (p - off[b]);
    std::memcpy(skey.data() + 32 * (size_t)p, to.key.data() + 32 * (size_t)src, 32);
    std::memcpy(slot.data() + 32 * (size_t)p, to.leaf.data() + 32 * (size_t)src, 32);
  }
  if (!levels(skey, slot, gathered, stl::kTreeBucketDepth)) return -2;
  // 6. bucket values and the top
  for (uint32_t b = 0; b < stl::kTreeBuckets; ++b) {
    if (dirty[b]) {
      to.bcnt[b] = sz[b];
      if (sz[b]) std::memcpy(&to.bh[8 * (size_t)b], slot.data() + 32 * (size_t)off[b], 32);
      else std::memset(&to.bh[8 * (size_t)b], 0, 32);
    } else {
      to.bcnt[b] = from.bcnt[b];
      std::memcpy(&to.bh[8 * (size_t)b], &from.bh[8 * (size_t)b], 32);
    }
  }
  std::vector<uint32_t> cc = to.bcnt, ch = to.bh;
  for (uint32_t nodes = 4096; nodes >= 1; nodes >>= 4) {
    std::vector<uint32_t> oc(nodes), oh(8 * (size_t)nodes);
    for (uint32_t t0 = 0; t0 < nodes; ++t0)
      oc[t0] = stl::shamap_tree_top_value(&cc[16 * (size_t)t0], &ch[128 * (size_t)t0], nodes == 1, &oh[8 * (size_t)t0]);
    cc.swap(oc);
    ch.swap(oh);
    if (nodes == 1) break;
  }
  if (cc[0] != m2) return -2;
  std::memcpy(to.root, ch.data(), 32);
  to.count = m2;
  // 7. finish, and the host's turn to the new generation
  std::memcpy(root, to.root, 32);
  if (counts) {
    const uint32_t c[8] = {m2, ins, rep, dele, absent, n - k, ndirty, gathered};
    std::memcpy(counts, c, 32);
  }
  t->live ^= 1;
  return 0;
}

}  // extern "C"
