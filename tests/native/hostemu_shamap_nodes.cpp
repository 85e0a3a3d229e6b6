// hostemu_shamap_nodes.cpp -- TEST HARNESS ONLY.  Compiles for the host what
// the node-storing calls (stl_shamap_nodes*, stl_shamap_tree_apply_nodes*) share
// with their kernels: the masking, leaf and meta rules of stl_shamap_core.h and
// the top-emission rules of stl_shamap_tree_core.h one by one, and both
// computations as stl_shamap.hip and stl_shamap_tree.hip stage them -- tiles of
// at most 128 nodes that take their row numbers with one add to a counter,
// every store guarded by the row number being below max_nodes -- on exactly
// sized heap arrays.  Not part of the product library.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../stellard_amd/csrc/stl_shamap_tree_core.h"

namespace {

void load(uint32_t w[8], const uint8_t* p) { stl::shamap_load_key(w, p, 0); }

// The caller's arrays (stl_shamap_nodes_out) and the counter the rows are numbered from.
struct Emit {
  uint32_t max_nodes;
  uint8_t *hash, *body, *id;
  uint32_t* meta;
  uint32_t counter = 0;
  void row(uint32_t at, const uint32_t h[8], const uint32_t* body_words, const uint32_t idw[8], uint32_t m) {
    if (at >= max_nodes) return;
    std::memcpy(hash + 32 * (size_t)at, h, 32);
    std::memcpy(body + 512 * (size_t)at, body_words, 512);
    if (id) std::memcpy(id + 32 * (size_t)at, idw, 32);
    if (meta) meta[at] = m;
  }
};

// Depths d_first down to d_last over m sorted keys with their slots, as the
// level kernel does (chunks of 256 positions, a chunk's records gathered before
// any slot is written); with emit, a chunk's nodes are stored as one tile.
// False when a chunk lists more than 128 nodes.
bool levels(const std::vector<uint8_t>& skey, std::vector<uint8_t>& slot, uint32_t m, uint32_t d_first,
            uint32_t d_last, Emit* emit, uint32_t hist_out[stl::kShamapDepths]) {
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
  if (hist_out) std::memcpy(hist_out, hist, sizeof(hist));
  for (int32_t d = (int32_t)d_first; d >= (int32_t)d_last; --d) {
    if (!hist[d]) continue;
    for (uint32_t t0 = 0; t0 < m; t0 += 256) {
      std::vector<uint32_t> pos;
      for (uint32_t i = t0; i < m && i < t0 + 256; ++i)
        if (stl::shamap_starts_node(i ? (int32_t)l[i - 1] : -1, (int32_t)l[i], d)) pos.push_back(i);
      if (pos.size() > 128) return false;
      if (pos.empty()) continue;
      uint32_t base = 0;
      if (emit) {
        base = emit->counter;
        emit->counter += (uint32_t)pos.size();
      }
      std::vector<uint32_t> rec(pos.size() * stl::kShamapRecordWords, 0u), leafs(pos.size(), 0u);
      for (size_t k = 0; k < pos.size(); ++k) {
        const uint32_t a = pos[k], e = stl::shamap_range_end(skey.data(), m, a, (uint32_t)d);
        uint32_t* r = rec.data() + k * stl::kShamapRecordWords;
        r[0] = stl::kShamapInnerPrefix;
        for (uint32_t c = 0; c < stl::kShamapBranches; ++c) {
          const uint32_t p = stl::shamap_branch_first(skey.data(), a, e, (uint32_t)d, c);
          if (p >= e) continue;
          std::memcpy(r + 1 + 8 * c, slot.data() + 32 * (size_t)p, 32);
          if (stl::shamap_branch_is_leaf(l.data(), p, e, (uint32_t)d)) leafs[k] |= 1u << c;
        }
      }
      for (size_t k = 0; k < pos.size(); ++k) {
        uint32_t h[8];
        const uint32_t* r = rec.data() + k * stl::kShamapRecordWords;
        stl::shamap_inner_hash(h, r);
        std::memcpy(slot.data() + 32 * (size_t)pos[k], h, 32);
        if (emit) {
          uint32_t key[8], id[8];
          load(key, skey.data() + 32 * (size_t)pos[k]);
          stl::shamap_mask_key(id, key, (uint32_t)d);
          emit->row(base + (uint32_t)k, h, r + 1, id, stl::shamap_node_meta((uint32_t)d, leafs[k]));
        }
      }
    }
  }
  return true;
}

}  // namespace

extern "C" {

void hostemu_nodes_mask_key(const uint8_t key[32], uint32_t d, uint8_t out[32]) {
  uint32_t w[8], o[8];
  load(w, key);
  stl::shamap_mask_key(o, w, d);
  std::memcpy(out, o, 32);
}

int hostemu_nodes_branch_is_leaf(const int8_t* l, uint32_t p, uint32_t e, uint32_t d) {
  return stl::shamap_branch_is_leaf(l, p, e, d) ? 1 : 0;
}

uint32_t hostemu_nodes_meta(uint32_t d, uint32_t leaf_mask) { return stl::shamap_node_meta(d, leaf_mask); }

int hostemu_nodes_top_emits(uint32_t cnt, int root, int dirty_below) {
  return stl::shamap_tree_top_emits(cnt, root != 0, dirty_below != 0) ? 1 : 0;
}

// cnt: 16 words; h: 16 * 32 bytes; body: 512 bytes; id: 32 bytes -> the leaf mask
uint32_t hostemu_nodes_top_node(const uint32_t* cnt, const uint8_t* h, uint32_t depth, uint32_t t, uint8_t* body,
                                uint8_t* id) {
  std::vector<uint32_t> hw(128), bw(128);
  std::memcpy(hw.data(), h, 512);
  uint32_t idw[8];
  const uint32_t leaf = stl::shamap_tree_top_node(cnt, hw.data(), depth, t, bw.data(), idw);
  std::memcpy(body, bw.data(), 512);
  std::memcpy(id, idw, 32);
  return leaf;
}

// stl_shamap_nodes as stl_shamap.hip stages it.  key, leaf (nullable): n * 32
// bytes; select (nullable): ceil(n / 8) bytes; root: 32 bytes; counts: 4 words;
// hash / body / id (nullable) / meta (nullable): max_nodes rows; count: one
// word.  Returns 0, or -1 when more than 128 nodes start in 256 positions.
int hostemu_nodes_set(const uint8_t* key, const uint8_t* leaf, const uint8_t* select, uint32_t n, uint8_t* root,
                      uint32_t* counts, uint32_t max_nodes, uint8_t* hash, uint8_t* body, uint8_t* id, uint32_t* meta,
                      uint32_t* count) {
  auto selected = [&](uint32_t r) { return !select || ((select[r >> 3] >> (r & 7u)) & 1u); };
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
    uint32_t x[8], y[8];
    load(x, key + 32 * (size_t)a);
    load(y, key + 32 * (size_t)b);
    return stl::shamap_key_less(x, y);
  });
  std::stable_partition(perm.begin(), perm.end(), selected);
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
  Emit emit{max_nodes, hash, body, id, meta};
  uint32_t hist[stl::kShamapDepths] = {};
  if (m && !levels(skey, slot, m, stl::kShamapDepths - 1, 0, &emit, hist)) return -1;
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
  *count = emit.counter;
  return 0;
}

// One stl_shamap_tree_apply_nodes to the tree that holds the m_old sorted keys
// old_key with leaf hashes old_leaf, as stl_shamap_tree.hip stages what it
// stores: the last of equal keys is a change, the changes are merged into the
// content, the dirty buckets' rows are gathered into a scratch whose depths 63
// down to 4 are hashed and stored, the clean buckets' values (the previous
// generation's, on the device) are hashed without storing, and the top is
// folded and stored by the top rules.  new_key / new_leaf: m_old + n rows of
// room; info: [0] the new count, [1] dirty buckets, [2] leaves gathered.
int hostemu_nodes_apply(const uint8_t* old_key, const uint8_t* old_leaf, uint32_t m_old, const uint8_t* key,
                        const uint8_t* leaf, const uint8_t* op, uint32_t n, uint8_t* new_key, uint8_t* new_leaf,
                        uint8_t* root, uint32_t* info, uint32_t max_nodes, uint8_t* hash, uint8_t* body, uint8_t* id,
                        uint32_t* meta, uint32_t* count) {
  if (n == 0) return -3;  // the report path stores nothing: the caller's business
  // 1. changes
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
    uint32_t x[8], y[8];
    load(x, key + 32 * (size_t)a);
    load(y, key + 32 * (size_t)b);
    return stl::shamap_key_less(x, y);
  });
  std::vector<uint32_t> change;  // rows, ascending by key
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t cp = 0;
    if (i + 1 < n) {
      uint32_t x[8], y[8];
      load(x, key + 32 * (size_t)perm[i]);
      load(y, key + 32 * (size_t)perm[i + 1]);
      cp = stl::shamap_common_prefix(x, y);
    }
    if (stl::shamap_tree_head(i + 1 == n, cp)) change.push_back(perm[i]);
  }
  // 2. / 3. the merge of two ascending sequences, and the dirty buckets
  std::vector<uint32_t> dirty(stl::kTreeBuckets, 0u);
  std::vector<uint8_t> nk, nl;
  uint32_t i = 0;
  auto push = [&](const uint8_t* k, const uint8_t* h) {
    nk.insert(nk.end(), k, k + 32);
    nl.insert(nl.end(), h, h + 32);
  };
  for (uint32_t row : change) {
    uint32_t w[8];
    const uint8_t* k = key + 32 * (size_t)row;
    load(w, k);
    dirty[stl::shamap_tree_bucket(w)] = 1u;
    bool found = false;
    const uint32_t p = stl::shamap_tree_lower_bound(old_key, m_old, w, &found);
    for (; i < p; ++i) push(old_key + 32 * (size_t)i, old_leaf + 32 * (size_t)i);
    if (found) ++i;
    if (!(op && op[row])) push(k, leaf ? leaf + 32 * (size_t)row : k);
  }
  for (; i < m_old; ++i) push(old_key + 32 * (size_t)i, old_leaf + 32 * (size_t)i);
  const uint32_t m2 = (uint32_t)(nk.size() / 32);
  if (m2) {
    std::memcpy(new_key, nk.data(), nk.size());
    std::memcpy(new_leaf, nl.data(), nl.size());
  }
  // 4. bucket bounds; 5. the dirty buckets' rows in a scratch, the others' in another
  std::vector<uint32_t> lb(stl::kTreeBuckets + 1);
  for (uint32_t b = 0; b <= stl::kTreeBuckets; ++b) lb[b] = stl::shamap_tree_bucket_begin(nk.data(), m2, b);
  std::vector<uint8_t> skey[2], slot[2];  // [1]: dirty
  std::vector<uint32_t> off(stl::kTreeBuckets);
  uint32_t ndirty = 0;
  for (uint32_t b = 0; b < stl::kTreeBuckets; ++b) {
    const int s = dirty[b] ? 1 : 0;
    ndirty += dirty[b];
    off[b] = (uint32_t)(skey[s].size() / 32);
    skey[s].insert(skey[s].end(), nk.begin() + 32 * (size_t)lb[b], nk.begin() + 32 * (size_t)lb[b + 1]);
    slot[s].insert(slot[s].end(), nl.begin() + 32 * (size_t)lb[b], nl.begin() + 32 * (size_t)lb[b + 1]);
  }
  const uint32_t gathered = (uint32_t)(skey[1].size() / 32);
  Emit emit{max_nodes, hash, body, id, meta};
  if (gathered && !levels(skey[1], slot[1], gathered, stl::kShamapDepths - 1, stl::kTreeBucketDepth, &emit, nullptr))
    return -1;
  if (!skey[0].empty() && !levels(skey[0], slot[0], (uint32_t)(skey[0].size() / 32), stl::kShamapDepths - 1,
                                  stl::kTreeBucketDepth, nullptr, nullptr))
    return -1;
  // 6. bucket values and the top
  std::vector<uint32_t> cc(stl::kTreeBuckets), ch(8 * (size_t)stl::kTreeBuckets, 0u), cd = dirty;
  for (uint32_t b = 0; b < stl::kTreeBuckets; ++b) {
    cc[b] = lb[b + 1] - lb[b];
    if (cc[b]) std::memcpy(&ch[8 * (size_t)b], slot[dirty[b] ? 1 : 0].data() + 32 * (size_t)off[b], 32);
  }
  uint32_t depth = stl::kTreeBucketDepth - 1;
  for (uint32_t nodes = 4096; nodes >= 1; nodes >>= 4, --depth) {
    std::vector<uint32_t> oc(nodes), oh(8 * (size_t)nodes), od(nodes);
    for (uint32_t t = 0; t < nodes; ++t) {
      const bool is_root = nodes == 1;
      oc[t] = stl::shamap_tree_top_value(&cc[16 * (size_t)t], &ch[128 * (size_t)t], is_root, &oh[8 * (size_t)t]);
      uint32_t below = 0;
      for (uint32_t k = 0; k < stl::kShamapBranches; ++k) below |= cd[16 * (size_t)t + k];
      od[t] = below ? 1u : 0u;
      if (!stl::shamap_tree_top_emits(oc[t], is_root, below != 0)) continue;
      uint32_t bw[128], idw[8];
      const uint32_t lm = stl::shamap_tree_top_node(&cc[16 * (size_t)t], &ch[128 * (size_t)t], depth, t, bw, idw);
      emit.row(emit.counter++, &oh[8 * (size_t)t], bw, idw, stl::shamap_node_meta(depth, lm));
    }
    cc.swap(oc);
    ch.swap(oh);
    cd.swap(od);
    if (nodes == 1) break;
  }
  if (cc[0] != m2) return -2;
  // 7. finish
  std::memcpy(root, ch.data(), 32);
  info[0] = m2;
  info[1] = ndirty;
  info[2] = gathered;
  *count = emit.counter;
  return 0;
}

}  // extern "C"
