// acctdir_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs the
// account directory's code (hostemu_acctdir.cpp over stl_acctdir_core.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, built and started by
// tests/test_acctdir_host.py.  Every array handed to the code is an exactly
// sized heap buffer, so a read or write outside it is an ASan report; the
// directory's own slots and records are exactly sized heap buffers too.
//
//   argv[1]  written by the test:
//            u64 seed, u32 k, k IDs that share a home slot near the end of a
//              256-slot table under that seed (the run wraps);
//            u32 n, n IDs, n flags bytes, n regular keys: the entries of the
//              blobs' accounts;
//            u32 b, then b times {u32 len, u32 authority, signer[20],
//              account[20], blob}: the whole blob must give those values
//              against the entries; every prefix of it a consistent row.
// Exit status = number of failed checks; any sanitizer report aborts.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "hostemu_acctdir.cpp"

static long g_bad = 0;
#define CHECK(c, ...)             \
  do {                            \
    if (!(c)) {                   \
      if (g_bad < 20) {           \
        std::printf(__VA_ARGS__); \
        std::printf("\n");        \
      }                           \
      ++g_bad;                    \
    }                             \
  } while (0)

static std::string slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// an exactly sized heap copy (NULL for nothing)
static uint8_t* exact(const uint8_t* src, size_t bytes) {
  if (!src) return nullptr;
  uint8_t* p = static_cast<uint8_t*>(std::malloc(bytes ? bytes : 1));
  if (bytes) std::memcpy(p, src, bytes);
  return p;
}

static int upsert_exact(void* d, const uint8_t* ids, const uint8_t* flags, const uint8_t* keys, size_t m) {
  uint8_t *a = exact(ids, 20 * m), *f = exact(flags, m), *k = exact(keys, 20 * m);
  const int rc = hostemu_acctdir_upsert(d, a, f, k, m);
  std::free(a);
  std::free(f);
  std::free(k);
  return rc;
}

// flags (m bytes) and, with want_keys, regular keys (20 m bytes) into `out`
static void lookup_exact(void* d, const uint8_t* ids, size_t m, bool want_keys, std::vector<uint8_t>& flags,
                         std::vector<uint8_t>& keys) {
  uint8_t* a = exact(ids, 20 * m);
  uint8_t* f = static_cast<uint8_t*>(std::malloc(m ? m : 1));
  uint8_t* k = want_keys ? static_cast<uint8_t*>(std::malloc(m ? 20 * m : 1)) : nullptr;
  hostemu_acctdir_lookup(d, a, m, f, k);
  flags.assign(f, f + m);
  keys.clear();
  if (k) keys.assign(k, k + 20 * m);
  std::free(a);
  std::free(f);
  std::free(k);
}

static uint32_t row_exact(void* d, const uint8_t* src, uint32_t len, uint8_t sg[20], uint8_t ac[20],
                          uint32_t* status) {
  uint8_t* heap = exact(src, len);
  const uint32_t auth = hostemu_acctdir_authority_row(d, heap, len, sg, ac, status);
  std::free(heap);
  return auth;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: %s acctdir.bin\n", argv[0]);
    return 251;
  }
  const std::string bin = slurp(argv[1]);
  const uint8_t* in = reinterpret_cast<const uint8_t*>(bin.data());
  size_t p = 0;
  auto need = [&](size_t bytes) {
    if (p + bytes > bin.size()) {
      std::printf("input truncated\n");
      std::exit(252);
    }
  };
  std::vector<uint8_t> fl, ks;
  uint32_t info[4];

  // ---- the same-home set: a run of k slots that wraps ----
  need(12);
  uint64_t seed;
  uint32_t k;
  std::memcpy(&seed, in + p, 8);
  std::memcpy(&k, in + p + 8, 4);
  p += 12;
  need(20 * (size_t)k);
  const uint8_t* home_ids = in + p;
  p += 20 * (size_t)k;
  {
    void* d = hostemu_acctdir_create(k, seed);
    std::vector<uint8_t> flags(k, stl::kAcctMasterDisabled);
    CHECK(upsert_exact(d, home_ids, flags.data(), nullptr, k) == 0, "same-home upsert");
    hostemu_acctdir_info(d, info);
    CHECK(info[1] == k && info[2] == stl::acctdir_slots(k) && info[3] == k, "same-home: records %u slots %u longest %u",
          info[1], info[2], info[3]);
    lookup_exact(d, home_ids, k, true, fl, ks);
    for (uint32_t i = 0; i < k; ++i) CHECK(fl[i] == stl::kAcctMasterDisabled, "same-home ID %u: flags %u", i, fl[i]);
    for (uint8_t b : ks) CHECK(b == 0, "same-home: a regular key without HAS_REGULAR_KEY");
    lookup_exact(d, home_ids, k, false, fl, ks);
    for (uint32_t i = 0; i < k; ++i) CHECK(fl[i] == stl::kAcctMasterDisabled, "same-home ID %u (no keys)", i);
    // strangers: the IDs with one bit changed
    std::vector<uint8_t> other(home_ids, home_ids + 20 * (size_t)k);
    for (uint32_t i = 0; i < k; ++i) other[20 * i + 7] ^= 0x10;
    lookup_exact(d, other.data(), k, true, fl, ks);
    for (uint32_t i = 0; i < k; ++i) CHECK(fl[i] == stl::kAcctNotFound, "stranger %u found", i);
    hostemu_acctdir_destroy(d);
    std::printf("same-home %u\n", k);

    // ---- capacity 1: four slots, one record ----
    d = hostemu_acctdir_create(1, seed);
    uint8_t f1 = stl::kAcctHasRegularKey;
    CHECK(upsert_exact(d, home_ids, &f1, home_ids + 20, 1) == 0, "capacity 1: first upsert");
    CHECK(upsert_exact(d, home_ids + 20, &f1, home_ids, 1) == -12, "capacity 1: a second account fits");
    uint8_t bad = 0x08;
    CHECK(upsert_exact(d, home_ids, &bad, home_ids, 1) == -22, "capacity 1: unknown flag bit accepted");
    CHECK(upsert_exact(d, home_ids, &f1, nullptr, 1) == -22, "capacity 1: HAS_REGULAR_KEY without keys accepted");
    lookup_exact(d, home_ids, 2, true, fl, ks);
    CHECK(fl[0] == f1 && fl[1] == stl::kAcctNotFound, "capacity 1: flags %u %u", fl[0], fl[1]);
    CHECK(!std::memcmp(ks.data(), home_ids + 20, 20), "capacity 1: regular key");
    hostemu_acctdir_info(d, info);
    CHECK(info[0] == 1 && info[1] == 1 && info[2] == 4 && info[3] == 1, "capacity 1: info");
    hostemu_acctdir_destroy(d);
  }

  // ---- the blobs' entries, then the blobs ----
  need(4);
  uint32_t n;
  std::memcpy(&n, in + p, 4);
  p += 4;
  need(41 * (size_t)n);
  const uint8_t *ids = in + p, *flags = ids + 20 * (size_t)n, *keys = flags + n;
  p += 41 * (size_t)n;
  void* d = hostemu_acctdir_create(n + 7, 0xABCDEFull);
  // in batches of 7, then all at once again (every row an update)
  for (uint32_t at = 0; at < n; at += 7) {
    const uint32_t m = n - at < 7 ? n - at : 7;
    CHECK(upsert_exact(d, ids + 20 * (size_t)at, flags + at, keys + 20 * (size_t)at, m) == 0, "entries at %u", at);
  }
  hostemu_acctdir_info(d, info);
  CHECK(info[1] == n, "entries: %u records of %u", info[1], n);
  CHECK(n <= 7 || upsert_exact(d, ids, flags, keys, n) == -12, "entries: a batch past the capacity was taken");
  CHECK(upsert_exact(d, ids, flags, keys, n < 7 ? n : 7) == 0, "entries: update");
  hostemu_acctdir_info(d, info);
  CHECK(info[1] == n, "entries: an update added records");
  lookup_exact(d, ids, n, true, fl, ks);
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t want = (flags[i] & stl::kAcctAbsent) ? (uint8_t)stl::kAcctNotFound : flags[i];
    CHECK(fl[i] == want, "entry %u: flags %u, want %u", i, fl[i], want);
    const bool has = want != stl::kAcctNotFound && (want & stl::kAcctHasRegularKey);
    uint8_t zero[20] = {0};
    CHECK(!std::memcmp(&ks[20 * (size_t)i], has ? keys + 20 * (size_t)i : zero, 20), "entry %u: regular key", i);
  }
  std::printf("entries %u\n", n);

  need(4);
  uint32_t nb;
  std::memcpy(&nb, in + p, 4);
  p += 4;
  size_t nblobs = 0;
  for (uint32_t j = 0; j < nb; ++j) {
    need(48);
    uint32_t len, want_auth;
    std::memcpy(&len, in + p, 4);
    std::memcpy(&want_auth, in + p + 4, 4);
    const uint8_t* want_sg = in + p + 8;
    const uint8_t* want_ac = want_sg + 20;
    const uint8_t* blob = want_ac + 20;
    need(48 + (size_t)len);
    uint8_t sg[20], ac[20], zero[20] = {0};
    uint32_t status = 99;
    const uint32_t auth = row_exact(d, blob, len, sg, ac, &status);
    CHECK(status == 0 && auth == want_auth && !std::memcmp(sg, want_sg, 20) && !std::memcmp(ac, want_ac, 20),
          "blob %u: status %u authority %u (want %u)", j, status, auth, want_auth);
    for (uint32_t c = 0; c <= len; ++c) {
      status = 99;
      const uint32_t a = row_exact(d, blob, c, sg, ac, &status);
      CHECK(a <= stl::kAuthUndecided && status <= 2, "prefix %u: authority %u status %u", c, a, status);
      if (status != 0)
        CHECK(a == stl::kAuthUndecided && !std::memcmp(sg, zero, 20) && !std::memcmp(ac, zero, 20),
              "prefix %u: status %u with a verdict or IDs", c, status);
    }
    p += 48 + (size_t)len;
    ++nblobs;
  }
  hostemu_acctdir_destroy(d);
  std::printf("blobs %zu\n", nblobs);
  CHECK(nblobs == 3, "expected 3 blobs");
  std::printf("failed checks %ld\n", g_bad);
  return g_bad > 250 ? 250 : (int)g_bad;
}
