// The device-side pieces the mesh operations share (mesh.hip, mesh_scan.hip, mesh_components.hip, mesh_simplify.hip, mesh_smooth.hip):
// the wave sum, keep masks and stable destinations, triple validation, the range test and quantisation of a position, the
// unit-vector emission and the open-addressed table.
#pragma once

#include "common.hpp"

namespace tsdf {

__device__ inline uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o);
        if ((int)lane >= o) v += up;
    }
    return v;
}

// One wave per chunk of 64 items: the chunk's keep mask and, as the count the chunk scan turns into a base, its popcount.
__device__ inline void store_keep_mask(bool keep, uint32_t lane, uint32_t chunk, uint64_t *__restrict__ mask, uint32_t *__restrict__ base) {
    const uint64_t m = __ballot(keep);
    if (lane == 0) {
        mask[chunk] = m;
        base[chunk] = (uint32_t)__popcll(m);
    }
}

// where kept item `at` goes: its chunk's base plus the kept items below it (at most 2^32 - 1 items: the sum fits)
__device__ inline uint32_t compact_index(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ base, uint32_t at) {
    return base[at >> 6] + (uint32_t)__popcll(mask[at >> 6] & ((1ull << (at & 63u)) - 1));
}

// The three indices of triple t; false when one of them is not below n_vertices, before any of them is an address.  The first kernel
// of a call that reads the indices then raises the call's error word, and the host reads the word before it returns.
__device__ inline bool load_triple(uint32_t n_vertices, const uint32_t *__restrict__ indices, uint64_t t, uint32_t c[3]) {
    c[0] = indices[3 * t];
    c[1] = indices[3 * t + 1];
    c[2] = indices[3 * t + 2];
    return !(c[0] >= n_vertices || c[1] >= n_vertices || c[2] >= n_vertices);
}

enum : unsigned long long { kErrorIndex = 1, kErrorTableFull = 2 };   // an error word's values; the larger one wins

__device__ inline void raise_error(uint64_t *error, unsigned long long code) { atomicMax((unsigned long long *)error, code); }

// A coordinate that quantises: |x| < 2^21 (false for NaN), so that x * 1024 is exact and below 2^31.
__device__ inline bool coordinate_in_range(float x) { return fabsf(x) < 2097152.0f; }
__device__ inline long long quantise_coordinate(float x) { return llrintf(x * 1024.0f); }

// the direction of an integer sum as a unit vector; quiet NaNs where the sum is zero
__device__ inline void store_unit_or_nan(float *__restrict__ out, double dx, double dy, double dz) {
    const double length = sqrt(dx * dx + dy * dy + dz * dz);
    const float none = __uint_as_float(0x7fc00000u);
    out[0] = length == 0.0 ? none : (float)(dx / length);
    out[1] = length == 0.0 ? none : (float)(dy / length);
    out[2] = length == 0.0 ? none : (float)(dz / length);
}

// ---- the open-addressed table: 2^bits 64-bit keys (mesh_table_bits in mesh_handle.hpp), all kEmptyKey before the first claim --------
constexpr unsigned long long kEmptyKey = ~0ull;   // no caller's key: a cell key has no bit 63, an edge key no 0xffffffff as its smaller end

// Claim or find `key`: true with its slot, false when the walk found no empty slot.  One compare-and-swap per probe, linear probing.
// No lane ever waits: a probe ends on "was empty" (the compare-and-swap has just claimed the slot) or "was my key", and anything else
// moves on to the next slot.  A slot, once it holds a key, holds it for the rest of the call; the callers put at most half as many keys
// in as there are slots, so an empty slot lies on every walk and the walk ends within keys + 1 probes whatever the other lanes do.  On
// top of that argument the loop is bounded by the table's size: every trip finishes or advances.
__device__ inline bool table_claim(unsigned long long *keys, uint32_t bits, unsigned long long key, uint64_t *slot_out) {
    const uint64_t mask = (1ull << bits) - 1;
    uint64_t slot = (key * 0x9E3779B97F4A7C15ull) >> (64 - bits);
    for (uint64_t tries = 0; tries <= mask; tries++) {
        const unsigned long long old = atomicCAS(keys + slot, kEmptyKey, key);
        if (old == kEmptyKey || old == key) {
            *slot_out = slot;
            return true;
        }
        slot = (slot + 1) & mask;
    }
    return false;   // (a table without an empty slot: not reachable at load <= 1/2)
}

}  // namespace tsdf
