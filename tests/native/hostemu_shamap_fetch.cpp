// hostemu_shamap_fetch.cpp -- TEST HARNESS ONLY.  Compiles the shared code of
// the fetch pack between two resident SHAMaps
// (stellard_amd/csrc/stl_shamap_fetch_core.h) for the host: the rules one by
// one, and a whole call as the kernels of stl_shamap_fetch.hip stage it, step by
// step on exactly sized heap arrays -- two generations of exactly their trees'
// item counts, two scratches of exactly the rows gathered (running sums stand
// in for the scans, a loop over the lanes for a grid, a counter for the atomic
// row numbers).  Not part of the product library.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stellard_amd/csrc/stl_shamap_fetch_core.h"

namespace {

using stl::kShamapRecordWords;
using stl::kTreeBuckets;

std::vector<uint32_t> exclusive_scan(const uint32_t* in, size_t n) {
  std::vector<uint32_t> out(n);
  uint32_t sum = 0;
  for (size_t i = 0; i < n; ++i) {
    out[i] = sum;
    sum += in[i];
  }
  return out;
}

void st8(uint8_t* p, size_t row, const uint32_t v[8]) {
  for (uint32_t i = 0; i < 8; ++i)
    for (uint32_t b = 0; b < 4; ++b) p[32 * row + 4 * i + b] = (uint8_t)(v[i] >> (8 * b));
}

// One generation as the call reads it: exactly m rows, the 65,536 bucket values.
struct Gen {
  const uint8_t *key, *leaf;
  const uint32_t* cnt;
  const uint8_t* h;
  uint32_t m;
};

// One side's scratch, exactly `rows` rows.
struct Scratch {
  std::vector<uint8_t> skey, slot;
  std::vector<int8_t> l;
  uint32_t hist[64] = {};
  uint32_t m = 0;
};

// Steps 2: the rows of the buckets with sz != 0, in order, and the neighbour bytes.
void gather(const Gen& g, const std::vector<uint32_t>& sz, Scratch* s) {
  const std::vector<uint32_t> begin = exclusive_scan(g.cnt, kTreeBuckets);
  const std::vector<uint32_t> off = exclusive_scan(sz.data(), kTreeBuckets);
  uint32_t total = off[kTreeBuckets - 1] + sz[kTreeBuckets - 1];
  if (total > g.m) total = g.m;
  s->m = total;
  s->skey.assign(32 * (size_t)total, 0);
  s->slot.assign(32 * (size_t)total, 0);
  s->l.assign(total, 0);
  for (uint32_t p = 0; p < total; ++p) {
    const uint32_t b = stl::shamap_diff_bucket_of(off.data(), p);
    uint32_t lo, hi;
    stl::shamap_lookup_range(begin[b], g.cnt[b], g.m, &lo, &hi);
    const uint32_t src = lo + (p - off[b]);
    if (src >= hi) continue;
    std::memcpy(&s->skey[32 * (size_t)p], g.key + 32 * (size_t)src, 32);
    std::memcpy(&s->slot[32 * (size_t)p], g.leaf + 32 * (size_t)src, 32);
  }
  for (uint32_t j = 0; j < total; ++j) {
    uint32_t a[8], b[8] = {};
    stl::shamap_load_key(a, s->skey.data(), j);
    int32_t lp = -1;
    if (j > 0) {
      stl::shamap_load_key(b, s->skey.data(), j - 1);
      lp = (int32_t)stl::shamap_common_prefix(b, a);
    }
    const bool last = j + 1 == total;
    if (!last) stl::shamap_load_key(b, s->skey.data(), j + 1);
    const int32_t lc = stl::shamap_neighbour(a, b, last, total == 1);
    s->l[j] = (int8_t)lc;
    for (int32_t d = lp + 1; d <= lc; ++d) ++s->hist[d];
  }
}

struct Node {
  uint32_t a, leaf;
  uint32_t rec[kShamapRecordWords], out[8];
};

// The nodes of depth d of a scratch, gathered and hashed; the slots are written
// by the caller once every node of the depth has read its own.
std::vector<Node> level(const Scratch& s, uint32_t d) {
  std::vector<Node> nodes;
  for (uint32_t i = 0; i < s.m; ++i) {
    if (!stl::shamap_starts_node(i ? (int32_t)s.l[i - 1] : -1, (int32_t)s.l[i], (int32_t)d)) continue;
    Node n{};
    n.a = i;
    const uint32_t e = stl::shamap_range_end(s.skey.data(), s.m, i, d);
    n.rec[0] = stl::kShamapInnerPrefix;
    for (uint32_t c = 0; c < 16; ++c) {
      const uint32_t p = stl::shamap_branch_first(s.skey.data(), i, e, d, c);
      uint32_t h[8] = {};
      if (p < e) {
        stl::shamap_load_key(h, s.slot.data(), p);
        if (stl::shamap_branch_is_leaf(s.l.data(), p, e, d)) n.leaf |= 1u << c;
      }
      for (uint32_t w = 0; w < 8; ++w) n.rec[1 + 8 * c + w] = h[w];
    }
    stl::shamap_inner_hash(n.out, n.rec);
    nodes.push_back(n);
  }
  return nodes;
}

}  // namespace

extern "C" {

uint32_t hostemu_fetch_want_rows(int differs, uint32_t cw) { return stl::shamap_fetch_want_rows(differs != 0, cw); }
uint32_t hostemu_fetch_have_rows(int differs, uint32_t cw, uint32_t ch) {
  return stl::shamap_fetch_have_rows(differs != 0, cw, ch);
}
int hostemu_fetch_top_inner(uint32_t cnt, int root) { return stl::shamap_fetch_top_inner(cnt, root != 0) ? 1 : 0; }
int hostemu_fetch_top_keeps(const uint8_t* hw, uint32_t ch, const uint8_t* hh, int root) {
  uint32_t x[8], y[8];
  stl::shamap_load_key(x, hw, 0);
  stl::shamap_load_key(y, hh, 0);
  return stl::shamap_fetch_top_keeps(x, ch, y, root != 0) ? 1 : 0;
}

// shamap_fetch_top_value against shamap_tree_top_value on 16 children: 1 when
// count and hash agree (and the record is the body whenever the value was hashed).
int hostemu_fetch_top_value_agrees(const uint32_t* cnt, const uint8_t* h, int root) {
  uint32_t hw[128], a[8], b[8], rec[kShamapRecordWords] = {};
  for (uint32_t c = 0; c < 16; ++c) stl::shamap_load_key(hw + 8 * c, h, c);
  const uint32_t ca = stl::shamap_tree_top_value(cnt, hw, root != 0, a);
  const uint32_t cb = stl::shamap_fetch_top_value(cnt, hw, root != 0, rec, b);
  if (ca != cb || std::memcmp(a, b, 32) != 0) return 0;
  if (stl::shamap_fetch_top_inner(cb, root != 0)) {
    uint32_t body[128], id[8];
    stl::shamap_tree_top_node(cnt, hw, 0, 0, body, id);
    if (std::memcmp(body, rec + 1, 512) != 0) return 0;
  }
  return 1;
}

// hasInnerNode over a scratch given as arrays (keys, neighbour bytes, slots).
int hostemu_fetch_have_holds(const uint8_t* hkey, const int8_t* hl, const uint8_t* hslot, uint32_t mh,
                             const uint8_t* id, uint32_t d, const uint8_t* hash) {
  uint32_t x[8], y[8];
  stl::shamap_load_key(x, id, 0);
  stl::shamap_load_key(y, hash, 0);
  return stl::shamap_fetch_have_holds(hkey, hl, hslot, mh, x, d, y) ? 1 : 0;
}

// The staged call.  want: wk / wl (mw sorted rows), wcnt / wh (the bucket
// values); have the same, or has_have = 0.  Rows go to hash / body / ids (or
// null) / meta (or null) below max_nodes only; *count and counts[8] at the end.
// 0, or -1 when a scratch read would leave its rows.
int hostemu_fetch_pack(const uint8_t* wk, const uint8_t* wl, const uint32_t* wcnt, const uint8_t* wh, uint32_t mw,
                       const uint8_t* hk, const uint8_t* hl, const uint32_t* hcnt, const uint8_t* hh, uint32_t mh,
                       int has_have, uint32_t max_nodes, uint8_t* hash, uint8_t* body, uint8_t* ids, uint32_t* meta,
                       uint32_t* count, uint32_t* counts) {
  const Gen want{wk, wl, wcnt, wh, mw};
  const std::vector<uint32_t> no_cnt(kTreeBuckets, 0u);
  const std::vector<uint8_t> no_h(32 * (size_t)kTreeBuckets, 0);
  const Gen have = has_have ? Gen{hk, hl, hcnt, hh, mh} : Gen{nullptr, nullptr, no_cnt.data(), no_h.data(), 0};
  uint32_t emitted = 0, buckets = 0, candidates = 0, suppressed = 0;
  auto store = [&](const uint32_t* h, const uint32_t* b, const uint32_t* id, uint32_t m) {
    const uint32_t row = emitted++;
    if (row >= max_nodes) return;
    st8(hash, row, h);
    for (uint32_t c = 0; c < 16; ++c) st8(body + 512 * (size_t)row, c, b + 8 * c);
    if (ids) st8(ids, row, id);
    if (meta) meta[row] = m;
  };
  // 1. buckets
  std::vector<uint32_t> sz_w(kTreeBuckets), sz_h(kTreeBuckets);
  for (uint32_t b = 0; b < kTreeBuckets; ++b) {
    uint32_t x[8], y[8];
    stl::shamap_load_key(x, want.h, b);
    stl::shamap_load_key(y, have.h, b);
    const bool differs = stl::shamap_bucket_differs(want.cnt[b], x, have.cnt[b], y);
    sz_w[b] = stl::shamap_fetch_want_rows(differs, want.cnt[b]);
    sz_h[b] = stl::shamap_fetch_have_rows(differs, want.cnt[b], have.cnt[b]);
    buckets += differs;
  }
  // 2. gather
  Scratch sw, sh;
  if (mw) gather(want, sz_w, &sw);
  if (mw && has_have && mh) gather(have, sz_h, &sh);
  // 3. levels
  for (int d = 63; d >= 4; --d) {
    if (sh.hist[d]) {
      const std::vector<Node> hn = level(sh, (uint32_t)d);
      for (const Node& n : hn) st8(sh.slot.data(), n.a, n.out);
    }
    if (!sw.hist[d]) continue;
    const std::vector<Node> wn = level(sw, (uint32_t)d);
    for (const Node& n : wn) {
      st8(sw.slot.data(), n.a, n.out);
      uint32_t key[8], id[8];
      stl::shamap_load_key(key, sw.skey.data(), n.a);
      stl::shamap_mask_key(id, key, (uint32_t)d);
      ++candidates;
      if (stl::shamap_fetch_have_holds(sh.skey.data(), sh.l.data(), sh.slot.data(), sh.m, id, (uint32_t)d, n.out)) {
        ++suppressed;
        continue;
      }
      store(n.out, n.rec + 1, id, stl::shamap_node_meta((uint32_t)d, n.leaf));
    }
  }
  // 4. top
  std::vector<uint32_t> wc(want.cnt, want.cnt + kTreeBuckets), hc(have.cnt, have.cnt + kTreeBuckets);
  std::vector<uint32_t> wv(8 * (size_t)kTreeBuckets), hv(8 * (size_t)kTreeBuckets);
  for (uint32_t b = 0; b < kTreeBuckets; ++b) {
    stl::shamap_load_key(&wv[8 * (size_t)b], want.h, b);
    stl::shamap_load_key(&hv[8 * (size_t)b], have.h, b);
  }
  for (uint32_t depth = 4; depth-- > 0;) {
    const uint32_t nodes = 1u << (4 * depth);
    const bool root = depth == 0;
    std::vector<uint32_t> nwc(nodes), nhc(nodes), nwv(8 * (size_t)nodes), nhv(8 * (size_t)nodes);
    for (uint32_t t = 0; t < nodes; ++t) {
      uint32_t rec[kShamapRecordWords];
      nhc[t] = 0u;
      if (has_have)
        nhc[t] = stl::shamap_fetch_top_value(&hc[16 * t], &hv[128 * (size_t)t], root, rec, &nhv[8 * (size_t)t]);
      nwc[t] = stl::shamap_fetch_top_value(&wc[16 * t], &wv[128 * (size_t)t], root, rec, &nwv[8 * (size_t)t]);
      if (!stl::shamap_fetch_top_inner(nwc[t], root)) continue;
      ++candidates;
      if (!stl::shamap_fetch_top_keeps(&nwv[8 * (size_t)t], nhc[t], &nhv[8 * (size_t)t], root)) {
        ++suppressed;
        continue;
      }
      uint32_t id[8];
      const uint32_t leaf = stl::shamap_tree_top_node(&wc[16 * t], &wv[128 * (size_t)t], depth, t, rec + 1, id);
      store(&nwv[8 * (size_t)t], rec + 1, id, stl::shamap_node_meta(depth, leaf));
    }
    wc.swap(nwc), hc.swap(nhc), wv.swap(nwv), hv.swap(nhv);
  }
  // 5. finish
  *count = emitted;
  counts[0] = emitted;
  counts[1] = buckets;
  counts[2] = sw.m;
  counts[3] = sh.m;
  counts[4] = candidates;
  counts[5] = suppressed;
  counts[6] = mw;
  counts[7] = has_have ? mh : 0u;
  return 0;
}

}  // extern "C"
