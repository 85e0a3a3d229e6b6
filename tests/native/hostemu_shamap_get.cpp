// hostemu_shamap_get.cpp -- TEST HARNESS ONLY.  Compiles the shared code of a
// resident SHAMap's answers by node ID (stellard_amd/csrc/stl_shamap_get_core.h)
// for the host: the rules one by one, and a whole call as the kernels of
// stl_shamap_get.hip stage it, step by step on exactly sized heap arrays -- a
// generation of exactly its tree's item count, a scratch of exactly the rows
// gathered, task arrays of exactly the tasks (running sums stand in for the
// scans, a loop over the lanes for a grid).  Not part of the product library.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stellard_amd/csrc/stl_shamap_fetch_core.h"
#include "../../stellard_amd/csrc/stl_shamap_get_core.h"

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

// The scratch, exactly the rows gathered.
struct Scratch {
  std::vector<uint8_t> skey, slot;
  std::vector<int8_t> l;
  std::vector<uint64_t> seen;
  std::vector<uint32_t> off;
  uint32_t hist[64] = {};
  uint32_t m = 0;
};

// Step 3: the rows of the buckets with sz != 0, in order, and the neighbour bytes.
void gather(const Gen& g, const std::vector<uint32_t>& begin, const std::vector<uint32_t>& sz, Scratch* s) {
  s->off = exclusive_scan(sz.data(), kTreeBuckets);
  uint32_t total = s->off[kTreeBuckets - 1] + sz[kTreeBuckets - 1];
  if (total > g.m) total = g.m;
  s->m = total;
  s->skey.assign(32 * (size_t)total, 0);
  s->slot.assign(32 * (size_t)total, 0);
  s->l.assign(total, 0);
  s->seen.assign(total, 0);
  for (uint32_t p = 0; p < total; ++p) {
    const uint32_t b = stl::shamap_diff_bucket_of(s->off.data(), p);
    uint32_t lo, hi;
    stl::shamap_lookup_range(begin[b], g.cnt[b], g.m, &lo, &hi);
    const uint32_t src = lo + (p - s->off[b]);
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

// The node at (d, a) of a scratch: its record, leaf mask and hash, from the slots as they are.
struct Node {
  uint32_t a, leaf;
  uint32_t rec[kShamapRecordWords], out[8];
};

Node node_at(const Scratch& s, uint32_t a, uint32_t d) {
  Node n{};
  n.a = a;
  const uint32_t e = stl::shamap_range_end(s.skey.data(), s.m, a, d);
  n.rec[0] = stl::kShamapInnerPrefix;
  for (uint32_t c = 0; c < 16; ++c) {
    const uint32_t p = stl::shamap_branch_first(s.skey.data(), a, e, d, c);
    uint32_t h[8] = {};
    if (p < e) {
      stl::shamap_load_key(h, s.slot.data(), p);
      if (stl::shamap_branch_is_leaf(s.l.data(), p, e, d)) n.leaf |= 1u << c;
    }
    for (uint32_t w = 0; w < 8; ++w) n.rec[1 + 8 * c + w] = h[w];
  }
  stl::shamap_inner_hash(n.out, n.rec);
  return n;
}

// The plain level kernel: every node of depth d hashed, then the slots written.
void level(Scratch* s, uint32_t d) {
  std::vector<Node> nodes;
  for (uint32_t i = 0; i < s->m; ++i)
    if (stl::shamap_starts_node(i ? (int32_t)s->l[i - 1] : -1, (int32_t)s->l[i], (int32_t)d))
      nodes.push_back(node_at(*s, i, d));
  for (const Node& n : nodes) st8(s->slot.data(), n.a, n.out);
}

uint32_t bucket_at(const uint8_t* key, uint32_t pos) {
  return ((uint32_t)key[32 * (size_t)pos] << 8) | key[32 * (size_t)pos + 1];
}

}  // namespace

extern "C" {

int hostemu_get_id_masked(const uint8_t* id, uint32_t depth) {
  uint32_t x[8];
  stl::shamap_load_key(x, id, 0);
  return stl::shamap_get_id_masked(x, depth) ? 1 : 0;
}
uint32_t hostemu_get_kind(uint32_t c, uint32_t depth, int parent_two) {
  return stl::shamap_get_kind(c, depth, parent_two != 0);
}
uint32_t hostemu_get_path_depth(int32_t second) { return stl::shamap_get_path_depth(second); }
uint32_t hostemu_get_path_status(int32_t best, uint32_t D) { return stl::shamap_get_path_status(best, D); }
uint32_t hostemu_get_top_index(uint32_t d, uint32_t t) { return stl::shamap_get_top_index(d, t); }
uint32_t hostemu_get_scratch_pos(uint32_t pos, uint32_t begin_b, uint32_t off_b) {
  return stl::shamap_get_scratch_pos(pos, begin_b, off_b);
}
uint32_t hostemu_get_branch_end(const uint8_t* skey, uint32_t p, uint32_t hi, uint32_t d) {
  return stl::shamap_get_branch_end(skey, p, hi, d);
}
// The range of (depth, id) over m sorted keys with their bucket counts -> lo, hi.
void hostemu_get_range(const uint8_t* key, const uint32_t* bcnt, uint32_t m, const uint8_t* id, uint32_t depth,
                       uint32_t* lo, uint32_t* hi) {
  const std::vector<uint32_t> begin = exclusive_scan(bcnt, kTreeBuckets);
  const stl::GetTree t{key, begin.data(), bcnt, m};
  uint32_t x[8];
  stl::shamap_load_key(x, id, 0);
  stl::shamap_get_range(t, x, depth, lo, hi);
}

// The bucket values of m sorted rows by the level rule over all keys: bcnt
// (65,536 words) and bh (65,536 x 32 bytes), for a caller that has only the rows.
void hostemu_get_bucket_values(const uint8_t* key, const uint8_t* leaf, uint32_t m, uint32_t* bcnt, uint8_t* bh) {
  std::memset(bcnt, 0, 4 * (size_t)kTreeBuckets);
  std::memset(bh, 0, 32 * (size_t)kTreeBuckets);
  for (uint32_t i = 0; i < m; ++i) ++bcnt[bucket_at(key, i)];
  if (!m) return;
  const Gen g{key, leaf, bcnt, bh, m};
  const std::vector<uint32_t> begin = exclusive_scan(bcnt, kTreeBuckets);
  const std::vector<uint32_t> sz(bcnt, bcnt + kTreeBuckets);
  Scratch s;
  gather(g, begin, sz, &s);  // every bucket: the whole tree
  for (int d = 63; d >= 4; --d)
    if (s.hist[d]) level(&s, (uint32_t)d);
  uint32_t at = 0;
  for (uint32_t b = 0; b < kTreeBuckets; ++b) {
    if (bcnt[b]) std::memcpy(bh + 32 * (size_t)b, &s.slot[32 * (size_t)at], 32);
    at += bcnt[b];
  }
}

// The staged call.  The generation: gk / gl (m sorted rows), gcnt / gh (the
// bucket values).  n requests: id, depth, mode (or null).  Answers: status,
// first, rows, leaf_key / leaf_hash (or null); rows go to hash / body / ids (or
// null) / meta (or null) below max_nodes only; *count and counts[8] at the end.
// info[0]: the scratch's rows, info[1]: the tasks.  0, or -1 when a task names
// a place outside the scratch.
int hostemu_get_nodes(const uint8_t* gk, const uint8_t* gl, const uint32_t* gcnt, const uint8_t* gh, uint32_t m,
                      const uint8_t* id, const uint8_t* depth, const uint8_t* mode, uint32_t n, uint8_t* status,
                      uint32_t* first, uint32_t* rows, uint8_t* leaf_key, uint8_t* leaf_hash, uint32_t max_nodes,
                      uint8_t* hash, uint8_t* body, uint8_t* ids, uint32_t* meta, uint32_t* count, uint32_t* counts,
                      uint32_t* info) {
  const Gen g{gk, gl, gcnt, gh, m};
  const std::vector<uint32_t> begin = exclusive_scan(gcnt, kTreeBuckets);
  const stl::GetTree t{gk, begin.data(), gcnt, m};
  uint32_t inner = 0, leafs = 0, other = 0, buckets = 0, distinct = 0;
  auto request = [&](uint32_t i, uint32_t* idw, uint32_t* md) {
    stl::shamap_load_key(idw, id, i);
    *md = mode ? mode[i] : stl::kGetFat;
  };
  // 1. ranges
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t idw[8], md, r = 0, lp = stl::kGetNoLeaf;
    request(i, idw, &md);
    const uint32_t st =
        stl::shamap_get_request(t, idw, depth[i], md, false, [](uint32_t, uint32_t, uint32_t) {}, &r, &lp);
    status[i] = (uint8_t)st;
    rows[i] = r;
    const uint32_t zero[8] = {};
    uint32_t v[8];
    if (leaf_key) {
      if (lp < m) stl::shamap_load_key(v, gk, lp);
      st8(leaf_key, i, lp < m ? v : zero);
    }
    if (leaf_hash) {
      if (lp < m) stl::shamap_load_key(v, gl, lp);
      st8(leaf_hash, i, lp < m ? v : zero);
    }
    inner += st == stl::kAtInner;
    leafs += st == stl::kAtLeaf || st == stl::kAtOtherLeaf;
    other += st == stl::kAtAbsent || st == stl::kAtEmptyRoot || st == stl::kAtInvalid;
  }
  uint32_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    first[i] = total;
    total += rows[i];
  }
  // 2. tasks: exactly the rows below max_nodes
  const uint32_t tasks = total < max_nodes ? total : max_nodes;
  std::vector<uint32_t> task_pos(tasks, 0u), mark(kTreeBuckets, 0u);
  std::vector<uint8_t> task_depth(tasks, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (rows[i] == 0 || first[i] >= tasks) continue;
    uint32_t idw[8], md, r = 0, lp = 0;
    request(i, idw, &md);
    stl::shamap_get_request(
        t, idw, depth[i], md, true,
        [&](uint32_t j, uint32_t d, uint32_t pos) {
          const uint32_t row = first[i] + j;
          if (j >= rows[i] || row >= tasks) return;
          task_pos[row] = pos;
          task_depth[row] = (uint8_t)d;
          if (d >= stl::kTreeBucketDepth && pos < m) mark[bucket_at(gk, pos)] = 1u;
        },
        &r, &lp);
  }
  // 3. gather
  std::vector<uint32_t> sz(kTreeBuckets);
  for (uint32_t b = 0; b < kTreeBuckets; ++b) {
    sz[b] = mark[b] ? gcnt[b] : 0u;
    buckets += mark[b] != 0;
  }
  Scratch s;
  if (tasks && m) gather(g, begin, sz, &s);
  info[0] = s.m;
  info[1] = tasks;
  int rc = 0;
  // 4. levels: before depth d is hashed, the bodies of the tasks of depth d and
  // the hashes of the tasks of depth d + 1
  auto task_at = [&](uint32_t r) -> uint32_t {
    const uint32_t pos = task_pos[r];
    if (pos >= m) return stl::kGetNoLeaf;
    const uint32_t b = bucket_at(gk, pos);
    if (!mark[b] || pos < begin[b]) return stl::kGetNoLeaf;
    const uint32_t a = stl::shamap_get_scratch_pos(pos, begin[b], s.off[b]);
    return a < s.m ? a : stl::kGetNoLeaf;
  };
  for (int d = 63; d >= 3; --d) {
    const bool bodies = d >= 4 && s.hist[d], hashes = d + 1 < 64 && s.hist[d + 1];
    for (uint32_t r = 0; r < tasks && (bodies || hashes); ++r) {
      const uint32_t td = task_depth[r];
      if (!((bodies && td == (uint32_t)d) || (hashes && td == (uint32_t)d + 1))) continue;
      const uint32_t a = task_at(r);
      if (a == stl::kGetNoLeaf) { rc = -1; continue; }
      if (td == (uint32_t)d + 1) {
        std::memcpy(hash + 32 * (size_t)r, &s.slot[32 * (size_t)a], 32);
        continue;
      }
      const Node nd = node_at(s, a, (uint32_t)d);
      uint32_t key[8], nid[8];
      stl::shamap_load_key(key, s.skey.data(), a);
      stl::shamap_mask_key(nid, key, (uint32_t)d);
      for (uint32_t c = 0; c < 16; ++c) st8(body + 512 * (size_t)r, c, nd.rec + 1 + 8 * c);
      if (ids) st8(ids, r, nid);
      if (meta) meta[r] = stl::shamap_node_meta((uint32_t)d, nd.leaf);
      if (!(s.seen[a] >> d & 1u)) ++distinct;
      s.seen[a] |= 1ull << d;
    }
    if (d >= 4 && s.hist[d]) level(&s, (uint32_t)d);
  }
  // 5. top: the folded values, then the rows of the tasks above the buckets
  if (tasks) {
    const uint32_t top_values = stl::kTreeTopValues + 1;
    std::vector<uint32_t> topcnt(top_values), toph(8 * (size_t)top_values), seen_top(top_values, 0u);
    std::vector<uint32_t> bh(8 * (size_t)kTreeBuckets);
    for (uint32_t b = 0; b < kTreeBuckets; ++b) stl::shamap_load_key(&bh[8 * (size_t)b], gh, b);
    const uint32_t *c = gcnt, *h = bh.data();
    uint32_t o = 0;
    for (uint32_t dep = 4; dep-- > 0;) {
      const uint32_t nodes = 1u << (4 * dep);
      for (uint32_t p = 0; p < nodes; ++p) {
        uint32_t rec[kShamapRecordWords];
        topcnt[o + p] =
            stl::shamap_fetch_top_value(c + 16 * p, h + 128 * (size_t)p, dep == 0, rec, &toph[8 * (size_t)(o + p)]);
      }
      c = &topcnt[o], h = &toph[8 * (size_t)o];
      o += nodes;
    }
    for (uint32_t r = 0; r < tasks; ++r) {
      const uint32_t d = task_depth[r], pos = task_pos[r];
      if (d >= stl::kTreeBucketDepth) continue;
      if (pos >= m) { rc = -1; continue; }
      const uint32_t p = d ? bucket_at(gk, pos) >> (4u * (stl::kTreeBucketDepth - d)) : 0u;
      uint32_t leaf = 0;
      for (uint32_t ch = 0; ch < 16; ++ch) {
        const uint32_t child = 16u * p + ch;
        const uint32_t cc = d == 3u ? gcnt[child] : topcnt[stl::shamap_get_top_index(d + 1u, child)];
        const uint32_t* hv =
            d == 3u ? &bh[8 * (size_t)child] : &toph[8 * (size_t)stl::shamap_get_top_index(d + 1u, child)];
        const uint32_t zero[8] = {};
        st8(body + 512 * (size_t)r, ch, cc ? hv : zero);
        if (cc == 1u) leaf |= 1u << ch;
      }
      const uint32_t own = stl::shamap_get_top_index(d, p);
      uint32_t key[8], nid[8];
      stl::shamap_load_key(key, gk, pos);
      stl::shamap_mask_key(nid, key, d);
      st8(hash, r, &toph[8 * (size_t)own]);
      if (ids) st8(ids, r, nid);
      if (meta) meta[r] = stl::shamap_node_meta(d, leaf);
      if (!seen_top[own]) ++distinct;
      seen_top[own] = 1u;
    }
  }
  // 6. finish
  *count = total;
  if (counts) {
    counts[0] = total;
    counts[1] = inner;
    counts[2] = leafs;
    counts[3] = other;
    counts[4] = buckets;
    counts[5] = s.m;
    counts[6] = distinct;
    counts[7] = m;
  }
  return rc;
}

}  // extern "C"
