// keyset_sanitize_main.cpp -- TEST HARNESS ONLY.  An executable that runs the
// host build of the keyset's device code (hostemu_keyset.cpp: the functions
// the gfx950 kernels of stl_keyset.hip run) under AddressSanitizer +
// UndefinedBehaviorSanitizer, built and started by tests/test_keyset_host.py.
//
//   keyset_sanitize_main ROWS
//   ROWS: nkeys(u32 LE) keys(nkeys * 32), then records
//         key_index(u32 LE) sig(64) msg(32) expected_1_0_18(1) expected_1_0_0(1)
// Builds every key's table and verifies every record under both policies.
// Exit status = number of disagreements (+ 1 for any limb-bound violation);
// any sanitizer report aborts.
#include <cstdio>
#include <cstdlib>

#include "hostemu_keyset.cpp"

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[1 << 12];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 100;
  const std::vector<uint8_t> in = slurp(argv[1]);
  if (in.size() < 4) return 101;
  uint32_t nkeys;
  std::memcpy(&nkeys, in.data(), 4);
  const size_t rec = 4 + 64 + 32 + 2, head = 4 + (size_t)nkeys * 32;
  if (nkeys == 0 || nkeys > 16 || in.size() <= head || (in.size() - head) % rec) return 101;
  const size_t n = (in.size() - head) / rec;
  std::vector<uint8_t> pk(in.begin() + 4, in.begin() + head), sig(n * 64), msg(n * 32);
  std::vector<uint32_t> idx(n);
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* r = &in[head + rec * i];
    std::memcpy(&idx[i], r, 4);
    std::memcpy(&sig[64 * i], r + 4, 64);
    std::memcpy(&msg[32 * i], r + 68, 32);
  }
  long bad = 0;
  for (uint32_t policy = 0; policy < 2; ++policy) {
    std::vector<uint8_t> bm((n + 7) / 8);
    const uint64_t viol = hostemu_keyset_verify_batch(pk.data(), nkeys, idx.data(), sig.data(), msg.data(), n,
                                                      bm.data(), policy);
    if (viol) {
      std::printf("limb-bound violations: %llu\n", (unsigned long long)viol);
      ++bad;
    }
    for (size_t i = 0; i < n; ++i) {
      const int got = (bm[i >> 3] >> (i & 7)) & 1, exp = in[head + rec * i + 100 + policy];
      if (got != exp) {
        std::printf("row %zu policy %u: keyset %d expected %d\n", i, policy, got, exp);
        ++bad;
      }
    }
  }
  std::printf("keys %u rows %zu checks %llu disagreements %ld\n", nkeys, n,
              (unsigned long long)hostemu_bound_checks(), bad);
  return bad > 250 ? 250 : (int)bad;
}
