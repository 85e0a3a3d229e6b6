// hostemu_shamap_fork.cpp -- TEST HARNESS ONLY.  The resident SHAMap's fork and
// revert compiled for the host: the read clamp of stl_shamap_tree_core.h on its
// own, and a whole fork as the kernels of stl_shamap_tree.hip stage it between
// two trees of different capacities -- every read of the source under the
// clamp, every store into the destination under its capacity, on exactly sized
// heap arrays -- the snapshot kernel unit by unit, and the host's revert state.
// An apply is the same staging with one tree on both sides.  Builds on the
// generations and the level passes of hostemu_shamap_tree.cpp.  Not part of
// the product library.
#include "hostemu_shamap_tree.cpp"

namespace {

// A tree as stl_api_shamap_tree.cpp keeps it.
struct FTree {
  Tree t;
  bool revertible = false;
};

FTree* ftree_new(uint32_t cap) {
  FTree* f = new FTree();
  f->t.cap = cap;
  for (Gen& g : f->t.g) {
    g.key.assign(32 * (size_t)cap, 0);
    g.leaf.assign(32 * (size_t)cap, 0);
    g.bcnt.assign(stl::kTreeBuckets, 0);
    g.bh.assign(8 * (size_t)stl::kTreeBuckets, 0);
  }
  return f;
}

void report(const Gen& g, uint8_t* root, uint32_t* counts) {
  std::memcpy(root, g.root, 32);
  if (counts) {
    std::memset(counts, 0, 32);
    counts[0] = g.count;
  }
}

// The snapshot kernel: unit t of each array, 16 bytes at a time.
int snapshot(const Gen& from, uint32_t from_cap, Gen& to, uint32_t cap, uint8_t* root, uint32_t* counts) {
  const uint32_t bound = stl::shamap_tree_readable(from.count, from_cap);  // the host's bound, exact here
  if (bound > cap) return -1;
  const uint32_t fixed_units = 2 * stl::kTreeBuckets;
  const uint32_t units = 2 * bound > fixed_units ? 2 * bound : fixed_units;
  const uint32_t grid = (units + 255) / 256 * 256;
  const uint32_t m = stl::shamap_tree_snapshot_rows(from.count, from_cap, cap);
  for (uint32_t t = 0; t < grid; ++t) {
    if (t < 2 * m) {
      std::memcpy(to.key.data() + 16 * (size_t)t, from.key.data() + 16 * (size_t)t, 16);
      std::memcpy(to.leaf.data() + 16 * (size_t)t, from.leaf.data() + 16 * (size_t)t, 16);
    }
    if (t < fixed_units) std::memcpy(&to.bh[4 * (size_t)t], &from.bh[4 * (size_t)t], 16);
    if (t < stl::kTreeBuckets / 4) std::memcpy(&to.bcnt[4 * (size_t)t], &from.bcnt[4 * (size_t)t], 16);
  }
  std::memcpy(to.root, from.root, 32);
  to.count = m;
  report(to, root, counts);
  return 0;
}

// One batch of n >= 1 rows: `from` (of a tree of from_cap) read, `to` (of a
// tree of cap) written.  0; -1: the result does not fit cap (only work arrays
// written); -2: an invariant fails.
int stage(const Gen& from, uint32_t from_cap, Gen& to, uint32_t cap, const uint8_t* key, const uint8_t* leaf,
          const uint8_t* op, uint32_t n, uint8_t* root, uint32_t* counts) {
  const uint32_t m = stl::shamap_tree_readable(from.count, from_cap);
  // 1. changes
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
  // 2. locate in the source's readable rows
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
  // 3. merge: the source's rows below m read, the destination's below cap written
  std::vector<uint8_t> written(m2 ? m2 : 1, 0);
  for (uint32_t i = 0; i < m; ++i) {
    bool hit = false;
    const uint32_t r = stl::shamap_tree_changes_before(pos.data(), code.data(), k, i, &hit);
    if (hit && (code[r] & stl::kTreeOpDelete)) continue;
    const uint32_t dst = stl::shamap_tree_item_dest(i, r < k ? scan[r] : total);
    if (dst >= cap || dst >= m2 || written[dst]++) return -2;
    std::memcpy(to.key.data() + 32 * (size_t)dst, from.key.data() + 32 * (size_t)i, 32);
    std::memcpy(to.leaf.data() + 32 * (size_t)dst,
                hit ? cleaf.data() + 32 * (size_t)r : from.leaf.data() + 32 * (size_t)i, 32);
  }
  for (uint32_t j = 0; j < k; ++j) {
    if (code[j] & (stl::kTreeOpDelete | stl::kTreeFound)) continue;
    const uint32_t dst = stl::shamap_tree_insert_dest(pos[j], scan[j]);
    if (dst >= cap || dst >= m2 || written[dst]++) return -2;
    std::memcpy(to.key.data() + 32 * (size_t)dst, ckey.data() + 32 * (size_t)j, 32);
    std::memcpy(to.leaf.data() + 32 * (size_t)dst, cleaf.data() + 32 * (size_t)j, 32);
  }
  for (uint32_t i = 0; i < m2; ++i)
    if (!written[i]) return -2;
  // 4. bucket bounds of the destination
  std::vector<uint32_t> lb(stl::kTreeBuckets + 1);
  for (uint32_t b = 0; b <= stl::kTreeBuckets; ++b) lb[b] = stl::shamap_tree_bucket_begin(to.key.data(), m2, b);
  // 5. the dirty buckets' subtrees
  std::vector<uint32_t> sz(stl::kTreeBuckets), off(stl::kTreeBuckets);
  uint32_t gathered = 0, ndirty = 0;
  for (uint32_t b = 0; b < stl::kTreeBuckets; ++b) {
    sz[b] = dirty[b] ? lb[b + 1] - lb[b] : 0u;
    off[b] = gathered;
    gathered += sz[b];
    ndirty += dirty[b];
  }
  if (gathered > cap) return -2;  // the scratch is the destination's
  std::vector<uint8_t> skey(32 * (size_t)gathered), slot(32 * (size_t)gathered);
  for (uint32_t p = 0; p < gathered; ++p) {
    const uint32_t b = (uint32_t)(std::upper_bound(off.begin(), off.end(), p) - off.begin()) - 1;
    const uint32_t src = lb[b] + (p - off[b]);
    std::memcpy(skey.data() + 32 * (size_t)p, to.key.data() + 32 * (size_t)src, 32);
    std::memcpy(slot.data() + 32 * (size_t)p, to.leaf.data() + 32 * (size_t)src, 32);
  }
  if (!levels(skey, slot, gathered, stl::kTreeBucketDepth)) return -2;
  // 6. bucket values (a clean bucket's copied under the source's clamp) and the top
  for (uint32_t b = 0; b < stl::kTreeBuckets; ++b) {
    if (dirty[b]) {
      to.bcnt[b] = sz[b];
      if (sz[b]) std::memcpy(&to.bh[8 * (size_t)b], slot.data() + 32 * (size_t)off[b], 32);
      else std::memset(&to.bh[8 * (size_t)b], 0, 32);
    } else {
      to.bcnt[b] = stl::shamap_tree_readable(from.bcnt[b], from_cap);
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
  // 7. finish
  std::memcpy(root, to.root, 32);
  if (counts) {
    const uint32_t c[8] = {m2, ins, rep, dele, absent, n - k, ndirty, gathered};
    std::memcpy(counts, c, 32);
  }
  return 0;
}

// The host's part: commit on success, a refused revert after a failure.
int finish(FTree* dst, int rc) {
  if (rc) {
    dst->revertible = false;
    return rc;
  }
  dst->t.live ^= 1;
  dst->revertible = true;
  return 0;
}

}  // namespace

extern "C" {

uint32_t hostemu_fork_readable(uint32_t stated, uint32_t from_cap) { return stl::shamap_tree_readable(stated, from_cap); }

uint32_t hostemu_fork_snapshot_rows(uint32_t stated, uint32_t from_cap, uint32_t to_cap) {
  return stl::shamap_tree_snapshot_rows(stated, from_cap, to_cap);
}

void* hostemu_fork_new(uint32_t cap) { return ftree_new(cap); }

void hostemu_fork_free(void* h) { delete static_cast<FTree*>(h); }

// key / leaf: capacity * 32 bytes -> the live generation's sorted content; root: 32 bytes; returns the count.
uint32_t hostemu_fork_export(void* h, uint8_t* key, uint8_t* leaf, uint8_t* root) {
  const FTree* f = static_cast<FTree*>(h);
  const Gen& g = f->t.g[f->t.live];
  const uint32_t m = stl::shamap_tree_readable(g.count, f->t.cap);
  std::memcpy(key, g.key.data(), 32 * (size_t)m);
  std::memcpy(leaf, g.leaf.data(), 32 * (size_t)m);
  std::memcpy(root, g.root, 32);
  return g.count;
}

// The live generation's stated count, as a broken device word would give it.
void hostemu_fork_state_count(void* h, uint32_t count) {
  FTree* f = static_cast<FTree*>(h);
  f->t.g[f->t.live].count = count;
}

int hostemu_fork_apply(void* h, const uint8_t* key, const uint8_t* leaf, const uint8_t* op, uint32_t n, uint8_t* root,
                       uint32_t* counts) {
  FTree* f = static_cast<FTree*>(h);
  if (n == 0) {  // changes nothing, the revert state included
    report(f->t.g[f->t.live], root, counts);
    return 0;
  }
  return finish(f, stage(f->t.g[f->t.live], f->t.cap, f->t.g[f->t.live ^ 1], f->t.cap, key, leaf, op, n, root, counts));
}

// src's live generation with the batch -> dst; -3: src == dst.
int hostemu_fork_fork(void* hs, void* hd, const uint8_t* key, const uint8_t* leaf, const uint8_t* op, uint32_t n,
                      uint8_t* root, uint32_t* counts) {
  const FTree* s = static_cast<FTree*>(hs);
  FTree* d = static_cast<FTree*>(hd);
  if (s == d || n > d->t.cap) return -3;
  const Gen& from = s->t.g[s->t.live];
  Gen& to = d->t.g[d->t.live ^ 1];
  if (n == 0) return finish(d, snapshot(from, s->t.cap, to, d->t.cap, root, counts));
  return finish(d, stage(from, s->t.cap, to, d->t.cap, key, leaf, op, n, root, counts));
}

// 0, or -3 where stl_shamap_tree_revert gives STL_EINVAL.
int hostemu_fork_revert(void* h) {
  FTree* f = static_cast<FTree*>(h);
  if (!f->revertible) return -3;
  f->t.live ^= 1;
  f->revertible = false;
  return 0;
}

}  // extern "C"
