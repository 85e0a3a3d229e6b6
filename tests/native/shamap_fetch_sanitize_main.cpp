// shamap_fetch_sanitize_main.cpp -- TEST HARNESS ONLY.  The staged fetch pack of
// hostemu_shamap_fetch.cpp as a stand-alone program, for AddressSanitizer and
// UBSan: tests/test_shamap_fetch_host.py compiles it with
// -fsanitize=address,undefined and runs it as a child process (never loaded
// into Python).  Every array is a heap array of exactly its size: a
// generation's rows are exactly the tree's items, the outputs exactly max_nodes
// rows.  The bucket values are made here, by the level rule over all keys.
//
// Input file: u32 cases; per case u32 mw, mw sorted keys, mw leaf hashes; u32
// has_have, u32 mh, keys, leaf hashes; u32 max_nodes; u32 expected nodes, each
// (u32 depth, 32 id, 32 hash) in (depth, id) order; 8 x u32 counts.
#include <algorithm>
#include <cstdio>
#include <string>

#include "hostemu_shamap_fetch.cpp"

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
      std::memset(dst, 0, n);
      return;
    }
    if (n) std::memcpy(dst, data.data() + at, n);
    at += n;
  }
};

// Exactly sized generation: rows, and the bucket values by the level rule.
struct OwnGen {
  std::vector<uint8_t> key, leaf, bh;
  std::vector<uint32_t> bcnt;
  uint32_t m = 0;
  void read(Reader& r) {
    m = r.u32();
    key.resize(32 * (size_t)m);
    leaf.resize(32 * (size_t)m);
    r.bytes(key.data(), key.size());
    r.bytes(leaf.data(), leaf.size());
    bcnt.assign(kTreeBuckets, 0u);
    bh.assign(32 * (size_t)kTreeBuckets, 0);
    for (uint32_t i = 0; i < m; ++i) ++bcnt[((uint32_t)key[32 * (size_t)i] << 8) | key[32 * (size_t)i + 1]];
    if (!m) return;
    const Gen g{key.data(), leaf.data(), bcnt.data(), bh.data(), m};
    Scratch s;
    gather(g, bcnt, &s);  // every bucket: the whole tree
    for (int d = 63; d >= 4; --d) {
      if (!s.hist[d]) continue;
      const std::vector<Node> nodes = level(s, (uint32_t)d);
      for (const Node& n : nodes) st8(s.slot.data(), n.a, n.out);
    }
    uint32_t at = 0;
    for (uint32_t b = 0; b < kTreeBuckets; ++b) {
      if (bcnt[b]) std::memcpy(&bh[32 * (size_t)b], &s.slot[32 * (size_t)at], 32);
      at += bcnt[b];
    }
  }
};

std::string row_key(uint32_t depth, const uint8_t* id, const uint8_t* hash) {
  std::string k(1, (char)depth);
  k.append(reinterpret_cast<const char*>(id), 32);
  k.append(reinterpret_cast<const char*>(hash), 32);
  return k;
}

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
    OwnGen want, have;
    want.read(r);
    const uint32_t has_have = r.u32();
    have.read(r);
    const uint32_t max_nodes = r.u32(), expect = r.u32();
    std::vector<std::string> expected(expect);
    for (uint32_t i = 0; i < expect; ++i) {
      const uint32_t depth = r.u32();
      uint8_t id[32], hash[32];
      r.bytes(id, 32);
      r.bytes(hash, 32);
      expected[i] = row_key(depth, id, hash);
    }
    uint32_t want_counts[8];
    for (uint32_t& w : want_counts) w = r.u32();
    if (!r.ok) break;
    std::vector<uint8_t> hash(32 * (size_t)max_nodes), body(512 * (size_t)max_nodes), ids(32 * (size_t)max_nodes);
    std::vector<uint32_t> meta(max_nodes);
    uint32_t count = 0xA5A5A5A5u, counts[8];
    const int rc = hostemu_fetch_pack(want.key.data(), want.leaf.data(), want.bcnt.data(), want.bh.data(), want.m,
                                      have.key.data(), have.leaf.data(), have.bcnt.data(), have.bh.data(), have.m,
                                      (int)has_have, max_nodes, hash.data(), body.data(), ids.data(), meta.data(),
                                      &count, counts);
    uint32_t bad = rc != 0 || count != expect || std::memcmp(counts, want_counts, sizeof(counts)) != 0;
    const uint32_t rows = count < max_nodes ? count : max_nodes;
    std::vector<std::string> got(rows);
    for (uint32_t i = 0; i < rows; ++i) {
      got[i] = row_key(meta[i] & 0xffu, &ids[32 * (size_t)i], &hash[32 * (size_t)i]);
      // the body hashes to the row's hash
      uint32_t rec[kShamapRecordWords], out[8];
      uint8_t h[32];
      rec[0] = stl::kShamapInnerPrefix;
      for (uint32_t ch = 0; ch < 16; ++ch) stl::shamap_load_key(rec + 1 + 8 * ch, &body[512 * (size_t)i], ch);
      stl::shamap_inner_hash(out, rec);
      st8(h, 0, out);
      bad += std::memcmp(h, &hash[32 * (size_t)i], 32) != 0;
    }
    std::sort(expected.begin(), expected.end());
    std::sort(got.begin(), got.end());
    bad += std::adjacent_find(got.begin(), got.end()) != got.end();  // every node once
    if (rows == expect) bad += got != expected;
    else bad += !std::includes(expected.begin(), expected.end(), got.begin(), got.end());
    std::printf("want %u have %s%u room %u rc %d nodes %u rows %u%s\n", want.m, has_have ? "" : "none ", have.m,
                max_nodes, rc, count, rows, bad ? " FAILED" : "");
    failed += bad != 0;
  }
  if (!r.ok) {
    std::printf("short input\n");
    return 3;
  }
  std::printf("cases %u failed checks %u\n", cases, failed);
  return failed ? 1 : 0;
}
