// stl_keyset.h -- launch interface between stl_api.cpp (host) and
// stl_keyset.hip (gfx950 device code): registered signer sets (stl_keyset_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace stl {

// Table geometry (stl_comb.h), for stl_keyset_get_info and the host's sizing.
struct KeysetGeometry {
  uint32_t window_bits, windows, rows_per_window, row_bytes;
};
KeysetGeometry keyset_geometry();
// words of one key's table / record, and of the build scratch of one key
size_t keyset_key_words();
size_t keyset_rec_words();
size_t keyset_scratch_words_per_key();

// A keyset on the device: nkeys + 1 records and tables, the last the base
// point's (built by the same kernels from B's encoding).
//   rec     (nkeys + 1) * keyset_rec_words()
//   tables  (nkeys + 1) * keyset_key_words(), zero-filled before the build (a
//           key that does not decode keeps zero rows, never read)
// launch_keyset_decode: d_pk holds nkeys + 1 encodings, B's last.
hipError_t launch_keyset_decode(const uint8_t* d_pk, uint32_t nkeys, uint32_t* rec, hipStream_t stream);
// Tables of records [first, first + count); scratch: count *
// keyset_scratch_words_per_key() words.
hipError_t launch_keyset_build(const uint32_t* rec, uint32_t first, uint32_t count, uint32_t* tables,
                               uint32_t* scratch, hipStream_t stream);
// One lane per signature; policy: core_policy().  A key_index >= nkeys gives
// bit 0 and reads no table.  counters (nullable): [0] += accept bits.
hipError_t launch_keyset_verify(const uint8_t* sig, const uint8_t* msg, const uint32_t* key_index, uint32_t n,
                                const uint32_t* rec, const uint32_t* tables, uint32_t nkeys, uint32_t policy,
                                uint64_t* bitmap, unsigned long long* counters, hipStream_t stream);

// ---- verify by public key (stl_keyset_map.h) ----
// The keyset's map on the device: mask + 1 slots, probed at most max_probe far.
struct KeysetMapDev {
  const uint32_t* slots;
  uint32_t mask, max_probe;
  uint64_t seed;
};
// One lane per row: key_index[i] = the index of pk[32 i ..] in the set, or
// 0xFFFFFFFF.  miss_count (nullable, zeroed by the caller): += the rows not
// found; miss_rows (nullable, n words, needs miss_count): their row numbers,
// appended wave by wave in the order the waves reserve their places.
hipError_t launch_keyset_lookup(const uint8_t* pk, uint32_t n, const KeysetMapDev& map, const uint32_t* rec,
                                uint32_t* key_index, uint32_t* miss_rows, uint32_t* miss_count,
                                hipStream_t stream);
// Rows rows[0 .. m) of sig / msg / pk copied to csig (64 B) / cmsg (32 B) /
// cpk (32 B) in list order.  Every pointer 16-byte aligned.
hipError_t launch_keyset_gather_rows(const uint32_t* rows, uint32_t m, const uint8_t* sig, const uint8_t* msg,
                                     const uint8_t* pk, uint8_t* csig, uint8_t* cmsg, uint8_t* cpk,
                                     hipStream_t stream);
// bitmap bit rows[j] |= cwords bit j, j < m (bitmap already holds a 0 there).
hipError_t launch_keyset_scatter_bits(const uint32_t* rows, uint32_t m, const uint64_t* cwords, uint64_t* bitmap,
                                      hipStream_t stream);

}  // namespace stl
