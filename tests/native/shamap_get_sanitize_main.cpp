// shamap_get_sanitize_main.cpp -- TEST HARNESS ONLY.  The staged call of
// hostemu_shamap_get.cpp as a stand-alone program, for AddressSanitizer and
// UBSan: tests/test_shamap_get_host.py compiles it with
// -fsanitize=address,undefined and runs it as a child process (never loaded
// into Python).  Every array is a heap array of exactly its size: the
// generation's rows are exactly the tree's items, the per-request arrays exactly
// n entries, the node arrays exactly max_nodes rows.  The bucket values are made
// here, by the level rule over all keys.
//
// Input file: u32 cases; per case u32 m, m sorted keys, m leaf hashes; u32 n,
// n ids, n depth bytes, u32 has_modes, n mode bytes; u32 max_nodes; expected:
// n status bytes, n x u32 first, n x u32 rows, u32 total, min(total, max_nodes)
// rows of (u32 depth, 32 id, 32 hash), 8 x u32 counts.
#include <cstdio>

#include "hostemu_shamap_get.cpp"

namespace {

struct Reader {
  std::vector<uint8_t> data;
  size_t at = 0;
  bool ok = true;
  uint32_t u32() {
    uint32_t v = 0;
    bytes(reinterpret_cast<uint8_t*>(&v), 4);
    return v;
  }
  void bytes(uint8_t* dst, size_t n) {
    if (at + n > data.size()) {
      ok = false;
      if (n) std::memset(dst, 0, n);
      return;
    }
    if (n) std::memcpy(dst, data.data() + at, n);
    at += n;
  }
  std::vector<uint8_t> take(size_t n) {
    std::vector<uint8_t> v(n);
    bytes(v.data(), n);
    return v;
  }
  std::vector<uint32_t> words(size_t n) {
    std::vector<uint32_t> v(n);
    for (uint32_t& w : v) w = u32();
    return v;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Reader r;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) r.data.insert(r.data.end(), buf, buf + n);
    std::fclose(f);
  }
  const uint32_t cases = r.u32();
  uint32_t failed = 0;
  for (uint32_t c = 0; c < cases && r.ok; ++c) {
    const uint32_t m = r.u32();
    const std::vector<uint8_t> key = r.take(32 * (size_t)m), leaf = r.take(32 * (size_t)m);
    const uint32_t n = r.u32();
    const std::vector<uint8_t> id = r.take(32 * (size_t)n), depth = r.take(n);
    const uint32_t has_modes = r.u32();
    const std::vector<uint8_t> mode = r.take(n);
    const uint32_t max_nodes = r.u32();
    const std::vector<uint8_t> want_status = r.take(n);
    const std::vector<uint32_t> want_first = r.words(n), want_rows = r.words(n);
    const uint32_t total = r.u32(), stored = total < max_nodes ? total : max_nodes;
    std::vector<uint32_t> want_depth(stored);
    std::vector<uint8_t> want_id(32 * (size_t)stored), want_hash(32 * (size_t)stored);
    for (uint32_t i = 0; i < stored; ++i) {
      want_depth[i] = r.u32();
      r.bytes(&want_id[32 * (size_t)i], 32);
      r.bytes(&want_hash[32 * (size_t)i], 32);
    }
    const std::vector<uint32_t> want_counts = r.words(8);
    if (!r.ok) break;
    std::vector<uint32_t> bcnt(kTreeBuckets);
    std::vector<uint8_t> bh(32 * (size_t)kTreeBuckets);
    hostemu_get_bucket_values(key.data(), leaf.data(), m, bcnt.data(), bh.data());
    std::vector<uint8_t> status(n), leaf_key(32 * (size_t)n), leaf_hash(32 * (size_t)n);
    std::vector<uint32_t> first(n), rows(n), meta(max_nodes);
    std::vector<uint8_t> hash(32 * (size_t)max_nodes), body(512 * (size_t)max_nodes), ids(32 * (size_t)max_nodes);
    uint32_t count = 0xA5A5A5A5u, counts[8], info[2];
    const int rc = hostemu_get_nodes(key.data(), leaf.data(), bcnt.data(), bh.data(), m, id.data(), depth.data(),
                                     has_modes ? mode.data() : nullptr, n, status.data(), first.data(), rows.data(),
                                     leaf_key.data(), leaf_hash.data(), max_nodes, hash.data(), body.data(),
                                     ids.data(), meta.data(), &count, counts, info);
    uint32_t bad = rc != 0 || count != total || std::memcmp(counts, want_counts.data(), sizeof(counts)) != 0;
    bad += status != want_status || first != want_first || rows != want_rows;
    for (uint32_t i = 0; i < stored; ++i) {
      bad += (meta[i] & 0xffu) != want_depth[i];
      bad += std::memcmp(&ids[32 * (size_t)i], &want_id[32 * (size_t)i], 32) != 0;
      bad += std::memcmp(&hash[32 * (size_t)i], &want_hash[32 * (size_t)i], 32) != 0;
      // the body hashes to the row's hash
      uint32_t rec[kShamapRecordWords], out[8];
      uint8_t h[32];
      rec[0] = stl::kShamapInnerPrefix;
      for (uint32_t ch = 0; ch < 16; ++ch) stl::shamap_load_key(rec + 1 + 8 * ch, &body[512 * (size_t)i], ch);
      stl::shamap_inner_hash(out, rec);
      st8(h, 0, out);
      bad += std::memcmp(h, &hash[32 * (size_t)i], 32) != 0;
    }
    std::printf("items %u requests %u room %u rc %d rows %u stored %u scratch %u tasks %u%s\n", m, n, max_nodes, rc,
                count, stored, info[0], info[1], bad ? " FAILED" : "");
    failed += bad != 0;
  }
  if (!r.ok) {
    std::printf("short input\n");
    return 3;
  }
  std::printf("cases %u failed checks %u\n", cases, failed);
  return failed ? 1 : 0;
}
