// keyset_map_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs
// the keyset's key -> index map (hostemu_keyset_map.cpp: the builder, hash and
// probe of stl_keyset_map.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, built and started by
// tests/test_keyset_map_host.py: the cases of that file, from a generator of
// its own.
//
//   * nkeys in {1, 2, 3, 255, 256, 257, 4096}, random keys, every tenth a
//     copy of an earlier one: every key probes to its first index, 1,000
//     random keys and every key with one bit flipped probe to not-found, the
//     slot count is a power of two >= 4 * nkeys;
//   * 64 keys of which 40, found by brute force over the hash, share a home
//     slot under seed 0: the builder takes a later seed, the longest probe
//     sequence stays within the bound, every lookup is right.
// Exit status = number of failed checks; any sanitizer report aborts.
#include <cstdio>
#include <cstdlib>

#include "hostemu_keyset_map.cpp"

static uint64_t g_rng = 0x9d2c5680f1a3b7e5ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static void rnd_key(uint8_t* k) {
  for (int i = 0; i < 4; ++i) {
    const uint64_t v = rnd();
    std::memcpy(k + 8 * i, &v, 8);
  }
}

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

// every key to its first index; strangers and one-bit neighbours to not-found
static void check_set(const std::vector<uint8_t>& pk, uint32_t nkeys, const char* what) {
  void* h = hostemu_keyset_map_build(pk.data(), nkeys);
  CHECK(h != nullptr, "%s: no map for %u keys", what, nkeys);
  if (!h) return;
  uint32_t info[4];
  hostemu_keyset_map_info(h, info);
  CHECK(info[0] >= 4 * nkeys && (info[0] & (info[0] - 1)) == 0, "%s: %u slots for %u keys", what, info[0], nkeys);
  CHECK(info[1] >= 1 && info[1] <= hostemu_keyset_map_bound(), "%s: longest probe %u", what, info[1]);
  std::map<std::array<uint8_t, 32>, uint32_t> first;
  for (uint32_t i = 0; i < nkeys; ++i) {
    std::array<uint8_t, 32> a;
    std::memcpy(a.data(), &pk[32 * (size_t)i], 32);
    first.emplace(a, i);
  }
  std::vector<uint32_t> out(nkeys);
  hostemu_keyset_map_probe(h, pk.data(), nkeys, out.data());
  for (uint32_t i = 0; i < nkeys; ++i) {
    std::array<uint8_t, 32> a;
    std::memcpy(a.data(), &pk[32 * (size_t)i], 32);
    CHECK(out[i] == first[a], "%s: key %u -> %u, first index %u", what, i, out[i], first[a]);
  }
  std::vector<uint8_t> other(pk.begin(), pk.begin() + 32 * (size_t)nkeys);
  for (uint32_t i = 0; i < nkeys; ++i) other[32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
  hostemu_keyset_map_probe(h, other.data(), nkeys, out.data());
  for (uint32_t i = 0; i < nkeys; ++i) {
    std::array<uint8_t, 32> a;
    std::memcpy(a.data(), &other[32 * (size_t)i], 32);
    if (!first.count(a)) CHECK(out[i] == hostemu_keyset_map_empty(), "%s: flipped key %u -> %u", what, i, out[i]);
  }
  std::vector<uint8_t> strangers(32 * 1000);
  for (int i = 0; i < 1000; ++i) rnd_key(&strangers[32 * (size_t)i]);
  out.resize(1000);
  hostemu_keyset_map_probe(h, strangers.data(), 1000, out.data());
  for (int i = 0; i < 1000; ++i) CHECK(out[i] == hostemu_keyset_map_empty(), "%s: stranger %d -> %u", what, i, out[i]);
  hostemu_keyset_map_free(h);
}

int main() {
  for (uint32_t nkeys : {1u, 2u, 3u, 255u, 256u, 257u, 4096u}) {
    std::vector<uint8_t> pk(32 * (size_t)nkeys);
    for (uint32_t i = 0; i < nkeys; ++i) {
      if (i > 0 && i % 10 == 9)
        std::memcpy(&pk[32 * (size_t)i], &pk[32 * (size_t)(rnd() % i)], 32);
      else
        rnd_key(&pk[32 * (size_t)i]);
    }
    check_set(pk, nkeys, "random");
  }
  // 64 keys -> 256 slots; 40 of them with one home slot under seed 0
  std::vector<uint8_t> pk(32 * 64);
  uint32_t have = 0;
  while (have < 40) {
    uint8_t k[32];
    rnd_key(k);
    if ((hostemu_keyset_map_hash(k, 0) & 255u) == 17u) std::memcpy(&pk[32 * (size_t)have++], k, 32);
  }
  for (; have < 64; ++have) rnd_key(&pk[32 * (size_t)have]);
  void* h = hostemu_keyset_map_build(pk.data(), 64);
  CHECK(h != nullptr, "adversarial: no map");
  if (h) {
    uint32_t info[4];
    hostemu_keyset_map_info(h, info);
    CHECK(info[0] == 256, "adversarial: %u slots", info[0]);
    CHECK(info[2] != 0 || info[3] != 0, "adversarial: seed 0 kept");
    CHECK(info[1] <= hostemu_keyset_map_bound(), "adversarial: longest probe %u", info[1]);
    hostemu_keyset_map_free(h);
  }
  check_set(pk, 64, "adversarial");
  std::printf("failed checks %ld\n", g_bad);
  return g_bad > 250 ? 250 : (int)g_bad;
}
