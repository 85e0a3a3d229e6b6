// hostemu_shamap_lookup.cpp -- TEST HARNESS ONLY.  Compiles the shared code of
// the resident SHAMap's read-only calls
// (stellard_amd/csrc/stl_shamap_lookup_core.h) for the host: the rules one by
// one, and a whole lookup and a whole compare as the kernels of
// stl_shamap_lookup.hip stage them, step by step on exactly sized heap arrays
// (running sums stand in for the scans, a loop over the lanes for a grid, a
// wave's ballot is assembled bit by bit).  Not part of the product library.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stellard_amd/csrc/stl_shamap_lookup_core.h"

namespace {

std::vector<uint32_t> exclusive_scan(const uint32_t* in, size_t n) {
  std::vector<uint32_t> out(n);
  uint32_t sum = 0;
  for (size_t i = 0; i < n; ++i) {
    out[i] = sum;
    sum += in[i];
  }
  return out;
}

}  // namespace

extern "C" {

void hostemu_lookup_range(uint32_t begin, uint32_t cnt, uint32_t m, uint32_t* lo, uint32_t* hi) {
  stl::shamap_lookup_range(begin, cnt, m, lo, hi);
}

uint32_t hostemu_lookup_lower_bound(const uint8_t* skey, uint32_t lo, uint32_t hi, const uint8_t* key, int* found) {
  uint32_t k[8];
  stl::shamap_load_key(k, key, 0);
  bool f = false;
  const uint32_t p = stl::shamap_lookup_lower_bound(skey, lo, hi, k, &f);
  *found = f ? 1 : 0;
  return p;
}

int hostemu_bucket_differs(uint32_t cnt_a, const uint8_t* h_a, uint32_t cnt_b, const uint8_t* h_b) {
  uint32_t x[8], y[8];
  stl::shamap_load_key(x, h_a, 0);
  stl::shamap_load_key(y, h_b, 0);
  return stl::shamap_bucket_differs(cnt_a, x, cnt_b, y) ? 1 : 0;
}

uint32_t hostemu_diff_rank_a(uint32_t i, uint32_t lb_b) { return stl::shamap_diff_rank_a(i, lb_b); }
uint32_t hostemu_diff_rank_b(uint32_t j, uint32_t ub_a) { return stl::shamap_diff_rank_b(j, ub_a); }
uint32_t hostemu_diff_kind_a(int found, int equal) { return stl::shamap_diff_kind_a(found != 0, equal != 0); }
uint32_t hostemu_diff_kind_b(int found) { return stl::shamap_diff_kind_b(found != 0); }
uint32_t hostemu_diff_bucket_of(const uint32_t* off, uint32_t p) { return stl::shamap_diff_bucket_of(off, p); }

uint32_t hostemu_diff_slot(const uint8_t* ka, const uint8_t* la, uint32_t a0, uint32_t a1, const uint8_t* kb,
                           const uint8_t* lb, uint32_t b0, uint32_t b1, uint32_t q, uint32_t* kind, uint32_t* row_a,
                           uint32_t* row_b) {
  return stl::shamap_diff_slot(ka, la, a0, a1, kb, lb, b0, b1, q, kind, row_a, row_b);
}

// The staged lookup: skey / sleaf m sorted rows, bcnt the 65,536 bucket counts;
// n queries -> ceil(n / 64) words, n leaf hashes (or null), n positions (or null).
void hostemu_lookup(const uint8_t* skey, const uint8_t* sleaf, const uint32_t* bcnt, uint32_t m, const uint8_t* qkey,
                    uint32_t n, uint64_t* words, uint8_t* leaf, uint32_t* position) {
  const std::vector<uint32_t> begin = exclusive_scan(bcnt, stl::kTreeBuckets);
  for (uint32_t wave = 0; wave < (n + 63) / 64; ++wave) {
    uint64_t bits = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t i = 64 * wave + lane;
      if (i >= n) continue;
      uint32_t key[8], lo, hi;
      stl::shamap_load_key(key, qkey, i);
      const uint32_t b = stl::shamap_tree_bucket(key);
      stl::shamap_lookup_range(begin[b], bcnt[b], m, &lo, &hi);
      bool found = false;
      const uint32_t p = stl::shamap_lookup_lower_bound(skey, lo, hi, key, &found);
      if (leaf) {
        if (found) std::memcpy(leaf + 32 * (size_t)i, sleaf + 32 * (size_t)p, 32);
        else std::memset(leaf + 32 * (size_t)i, 0, 32);
      }
      if (position) position[i] = found ? p : stl::kDiffNoRow;
      if (found) bits |= 1ull << lane;
    }
    words[wave] = bits;
  }
}

// The staged compare of (ka, la, cnt_a, h_a; ma items) and (kb, ..; mb items):
// steps 1 to 4 of stl_shamap_lookup.hip with the workspace sized for ma + mb slots.
// 0, or negative when a slot's rank falls outside its bucket (-1), is taken
// twice (-2) or a slot stays unwritten (-3).
int hostemu_compare(const uint8_t* ka, const uint8_t* la, const uint32_t* cnt_a, const uint8_t* h_a, uint32_t ma,
                     const uint8_t* kb, const uint8_t* lb, const uint32_t* cnt_b, const uint8_t* h_b, uint32_t mb,
                     uint32_t max_rows, uint8_t* key, uint8_t* kind, uint8_t* leaf_a, uint8_t* leaf_b,
                     uint32_t* counts) {
  const uint32_t slots = ma + mb;
  uint32_t hdr[4] = {};
  // 1. buckets
  std::vector<uint32_t> sz(stl::kTreeBuckets);
  for (uint32_t b = 0; b < stl::kTreeBuckets; ++b) {
    uint32_t x[8], y[8];
    stl::shamap_load_key(x, h_a, b);
    stl::shamap_load_key(y, h_b, b);
    const bool differs = stl::shamap_bucket_differs(cnt_a[b], x, cnt_b[b], y);
    sz[b] = differs ? cnt_a[b] + cnt_b[b] : 0u;
    hdr[3] += differs;
  }
  const std::vector<uint32_t> begin_a = exclusive_scan(cnt_a, stl::kTreeBuckets);
  const std::vector<uint32_t> begin_b = exclusive_scan(cnt_b, stl::kTreeBuckets);
  const std::vector<uint32_t> off = exclusive_scan(sz.data(), stl::kTreeBuckets);
  uint32_t total = off[stl::kTreeBuckets - 1] + sz[stl::kTreeBuckets - 1];
  if (total > slots) total = slots;
  // 2. slots: exactly sized, and every one must be written exactly once
  std::vector<uint32_t> flag(total), row_a(total), row_b(total), written(total, 0u);
  for (uint32_t p = 0; p < total; ++p) {
    const uint32_t b = stl::shamap_diff_bucket_of(off.data(), p), q = p - off[b];
    uint32_t a0, a1, b0, b1, k = 0, ra = 0, rb = 0;
    stl::shamap_lookup_range(begin_a[b], cnt_a[b], ma, &a0, &a1);
    stl::shamap_lookup_range(begin_b[b], cnt_b[b], mb, &b0, &b1);
    if (q >= (a1 - a0) + (b1 - b0)) continue;
    const uint32_t s = off[b] + stl::shamap_diff_slot(ka, la, a0, a1, kb, lb, b0, b1, q, &k, &ra, &rb);
    if (s >= total) return -1;
    if (written[s]++) return -2;  // the ranks of a bucket are a permutation
    flag[s] = k != stl::kDiffNone;
    row_a[s] = ra;
    row_b[s] = rb;
    if (k) ++hdr[k - 1];
  }
  for (uint32_t p = 0; p < total; ++p)
    if (!written[p]) return -3;
  // 3. rows
  const std::vector<uint32_t> scan = exclusive_scan(flag.data(), total);
  for (uint32_t p = 0; p < total; ++p) {
    if (!flag[p] || scan[p] >= max_rows) continue;
    const uint32_t row = scan[p];
    const bool in_a = row_a[p] < ma, in_b = row_b[p] < mb;
    std::memcpy(key + 32 * (size_t)row, in_a ? ka + 32 * (size_t)row_a[p] : kb + 32 * (size_t)row_b[p], 32);
    kind[row] = (uint8_t)(in_a ? (in_b ? stl::kDiffChanged : stl::kDiffAOnly) : stl::kDiffBOnly);
    if (leaf_a) {
      if (in_a) std::memcpy(leaf_a + 32 * (size_t)row, la + 32 * (size_t)row_a[p], 32);
      else std::memset(leaf_a + 32 * (size_t)row, 0, 32);
    }
    if (leaf_b) {
      if (in_b) std::memcpy(leaf_b + 32 * (size_t)row, lb + 32 * (size_t)row_b[p], 32);
      else std::memset(leaf_b + 32 * (size_t)row, 0, 32);
    }
  }
  // 4. finish
  counts[0] = total ? scan[total - 1] + flag[total - 1] : 0u;
  counts[1] = hdr[0];
  counts[2] = hdr[1];
  counts[3] = hdr[2];
  counts[4] = hdr[3];
  counts[5] = total;
  counts[6] = ma;
  counts[7] = mb;
  return 0;
}

}  // extern "C"
