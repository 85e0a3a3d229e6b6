// signer_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs the
// signer-authority code (hostemu_signer.cpp: Hash160 of stl_hash160.h and the
// per-row function of stl_signer_core.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, built and started by tests/test_signer_host.py.
//
//   argv[1]  tests/golden/hash160_vectors.json: every key's SHA-256-of-32 is
//            fed to RIPEMD-160-of-32 and hash160_32 and compared with the
//            file's digests;
//   argv[2]  blobs written by the test, each {u32 len, u32 authority,
//            signer[20], account[20], blob}: the whole blob must give those
//            values; then every prefix of it, and the blob with each of its
//            first 80 bytes set to 0xff, is copied into an exactly sized heap
//            buffer and run -- a read outside [blob, blob + len) is an ASan
//            report -- and must give a consistent row (authority in range,
//            zero IDs on a row that is not STL_TX_OK).
// Exit status = number of failed checks; any sanitizer report aborts.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "hostemu_signer.cpp"

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

static int nib(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

// the hex strings of the JSON array named `name`
static std::vector<std::vector<uint8_t>> hex_array(const std::string& doc, const char* name) {
  std::vector<std::vector<uint8_t>> out;
  size_t p = doc.find(std::string("\"") + name + "\": [");
  if (p == std::string::npos) return out;
  p = doc.find('[', p);
  const size_t end = doc.find(']', p);
  while (true) {
    const size_t a = doc.find('"', p + 1);
    if (a == std::string::npos || a > end) break;
    const size_t b = doc.find('"', a + 1);
    std::vector<uint8_t> v;
    for (size_t i = a + 1; i + 1 < b; i += 2) v.push_back((uint8_t)(nib(doc[i]) * 16 + nib(doc[i + 1])));
    out.push_back(v);
    p = b;
  }
  return out;
}

// one run on an exactly sized heap copy
static uint32_t run_exact(const uint8_t* src, uint32_t len, uint8_t sg[20], uint8_t ac[20], uint32_t* status) {
  uint8_t* heap = static_cast<uint8_t*>(std::malloc(len ? len : 1));
  if (len) std::memcpy(heap, src, len);
  const uint32_t auth = hostemu_signer_row(heap, len, sg, ac, status);
  std::free(heap);
  return auth;
}

static void check_consistent(const uint8_t* src, uint32_t len, const char* what, uint32_t k) {
  uint8_t sg[20], ac[20], zero[20] = {0};
  uint32_t status = 99;
  const uint32_t auth = run_exact(src, len, sg, ac, &status);
  CHECK(auth <= 2 && status <= 2, "%s %u: authority %u status %u", what, k, auth, status);
  if (status != 0) {
    CHECK(auth == 2 && !std::memcmp(sg, zero, 20) && !std::memcmp(ac, zero, 20), "%s %u: status %u with IDs", what, k,
          status);
  } else if (auth != 2) {
    CHECK((auth == 1) == (std::memcmp(sg, ac, 20) == 0), "%s %u: authority %u against the IDs", what, k, auth);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("usage: %s hash160_vectors.json blobs.bin\n", argv[0]);
    return 251;
  }
  const std::string doc = slurp(argv[1]);
  const auto keys = hex_array(doc, "keys"), rmd = hex_array(doc, "ripemd160"), h160 = hex_array(doc, "hash160");
  CHECK(keys.size() >= 800 && rmd.size() == keys.size() && h160.size() == keys.size(), "fixture: %zu keys",
        keys.size());
  for (size_t i = 0; i < keys.size() && i < rmd.size() && i < h160.size(); ++i) {
    if (keys[i].size() != 32 || rmd[i].size() != 20 || h160[i].size() != 20) {
      CHECK(false, "fixture row %zu", i);
      continue;
    }
    uint8_t* k = static_cast<uint8_t*>(std::malloc(32));
    uint8_t* o = static_cast<uint8_t*>(std::malloc(20));
    std::memcpy(k, keys[i].data(), 32);
    hostemu_ripemd160_32(k, o);
    CHECK(!std::memcmp(o, rmd[i].data(), 20), "key %zu: RIPEMD-160", i);
    hostemu_hash160_32(k, 1, o);
    CHECK(!std::memcmp(o, h160[i].data(), 20), "key %zu: Hash160", i);
    std::free(k);
    std::free(o);
  }
  std::printf("keys %zu\n", keys.size());

  const std::string bin = slurp(argv[2]);
  size_t p = 0, nblobs = 0;
  while (p + 48 <= bin.size()) {
    uint32_t len, want_auth;
    std::memcpy(&len, &bin[p], 4);
    std::memcpy(&want_auth, &bin[p + 4], 4);
    const uint8_t* want_sg = reinterpret_cast<const uint8_t*>(&bin[p + 8]);
    const uint8_t* want_ac = want_sg + 20;
    const uint8_t* blob = want_ac + 20;
    if (p + 48 + len > bin.size()) {
      CHECK(false, "blob file truncated");
      break;
    }
    uint8_t sg[20], ac[20];
    uint32_t status = 99;
    const uint32_t auth = run_exact(blob, len, sg, ac, &status);
    CHECK(status == 0 && auth == want_auth && !std::memcmp(sg, want_sg, 20) && !std::memcmp(ac, want_ac, 20),
          "blob %zu: status %u authority %u (want %u)", nblobs, status, auth, want_auth);
    for (uint32_t k = 0; k <= len; ++k) check_consistent(blob, k, "prefix", k);
    std::vector<uint8_t> m(blob, blob + len);
    for (uint32_t k = 0; k < 80 && k < len; ++k) {
      const uint8_t keep = m[k];
      m[k] = 0xff;
      check_consistent(m.data(), len, "0xff at", k);
      m[k] = keep;
    }
    p += 48 + len;
    ++nblobs;
  }
  std::printf("blobs %zu\n", nblobs);
  CHECK(nblobs == 3, "expected 3 blobs");
  std::printf("failed checks %ld\n", g_bad);
  return g_bad > 250 ? 250 : (int)g_bad;
}
