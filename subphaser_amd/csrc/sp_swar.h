// sp_swar.h -- two 16-bit counters per 32-bit word: the write-out arithmetic of c2_count16 on both halves of a word at once.
//
// c2_count16 keeps its counters two to a word and writes 2^15 slots out per bucket; per slot it needs "count >= lower"
// (tallies n and s), min(count, 255) (the table byte) and "count >= 255" (the overflow list, rare).  Done slot by slot that
// was over half of the kernel's instructions.  Everything here is plain integer arithmetic, __host__ __device__, so that
// tests/test_swar_host.py checks it against the per-slot definition with the host compiler; where gfx950 has an instruction
// for a step (v_pk_min_u16, v_pk_max_u16, v_dot2_u32_u16, v_perm_b32) the device build uses it and the host build the
// portable form of the same function.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_SWAR_HD __host__ __device__ __forceinline__
#else
#define SP_SWAR_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short sp_swar_us2 __attribute__((ext_vector_type(2)));
#endif

// largest `lower` the flag trick below takes (a larger one goes through the per-slot code)
#define SP_SWAR_MAX_LOWER 0x8000u

// the same 16-bit value in both halves
SP_SWAR_HD uint32_t sp_swar_rep16(uint32_t v) { return (v & 0xffffu) | (v << 16); }

// bit 15 (bit 31) of the result is set iff the low (high) counter of w is >= lower; L2 = sp_swar_rep16(lower),
// 1 <= lower <= 0x8000.  A counter with bit 15 set is >= lower whatever lower is; for the others (c | 0x8000) - lower
// keeps bit 15 iff c >= lower and never borrows from the half above.
SP_SWAR_HD uint32_t sp_swar_ge_flags(uint32_t w, uint32_t L2) {
    const uint32_t t = ((w & 0x7fff7fffu) | 0x80008000u) - L2;
    return (t | w) & 0x80008000u;
}
// number of flagged counters
SP_SWAR_HD uint32_t sp_swar_flag_count(uint32_t flags) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_popcount(flags);
#else
    return (flags >> 15 & 1u) + (flags >> 31);
#endif
}
// acc + the flagged counters of w
SP_SWAR_HD uint32_t sp_swar_flag_sum(uint32_t w, uint32_t flags, uint32_t acc) {
    const uint32_t f = flags >> 15;      // 0 / 1 per half
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot2(__builtin_bit_cast(sp_swar_us2, w), __builtin_bit_cast(sp_swar_us2, f), acc, false);
#else
    return acc + (w & 0xffffu) * (f & 1u) + (w >> 16) * (f >> 16);
#endif
}
// per half: min / max
SP_SWAR_HD uint32_t sp_swar_min16(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(sp_swar_us2, a), __builtin_bit_cast(sp_swar_us2, b)));
#else
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al < bl ? al : bl) | ((ah < bh ? ah : bh) << 16);
#endif
}
SP_SWAR_HD uint32_t sp_swar_max16(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(sp_swar_us2, a), __builtin_bit_cast(sp_swar_us2, b)));
#else
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al : bl) | ((ah > bh ? ah : bh) << 16);
#endif
}
// the table bytes of the four counters of two words: min(c, 255) of a.low, a.high, b.low, b.high in bytes 0..3
SP_SWAR_HD uint32_t sp_swar_sat_bytes(uint32_t a, uint32_t b) {
    const uint32_t ma = sp_swar_min16(a, 0x00ff00ffu), mb = sp_swar_min16(b, 0x00ff00ffu);
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(mb, ma, 0x06040200u);
#else
    return (ma & 0xffu) | ((ma >> 16) << 8) | ((mb & 0xffu) << 16) | ((mb >> 16) << 24);
#endif
}
// nonzero iff one of the eight counters of the four words is >= 255 (min(max, 255) + 1 reaches bit 8 of its half)
SP_SWAR_HD uint32_t sp_swar_any_ge255(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t mx = sp_swar_max16(sp_swar_max16(a, b), sp_swar_max16(c, d));
    return (sp_swar_min16(mx, 0x00ff00ffu) + 0x00010001u) & 0x01000100u;
}

// ---- eight bytes per 64-bit word (the pair comparison of aligned rows, sp_domalign.hip)
// bit 7 of a byte of the result is set iff that byte of w is below 20 (a residue code).  (x & 0x7f) + 108 reaches bit 7
// iff the low seven bits are >= 20, and a byte with bit 7 set is >= 128; no carry leaves a byte: 127 + 108 < 256.
SP_SWAR_HD uint64_t sp_swar_lt20_bytes(uint64_t w) {
    const uint64_t t = (w & 0x7f7f7f7f7f7f7f7fULL) + 0x6c6c6c6c6c6c6c6cULL;
    return ~(t | w) & 0x8080808080808080ULL;
}
// bit 7 of a byte of the result is set iff that byte of a equals that byte of b: (x & 0x7f) + 127 reaches bit 7 iff the
// low seven bits of x = a ^ b are not all zero
SP_SWAR_HD uint64_t sp_swar_eq_bytes(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b, t = (x & 0x7f7f7f7f7f7f7f7fULL) + 0x7f7f7f7f7f7f7f7fULL;
    return ~(t | x) & 0x8080808080808080ULL;
}
// number of flagged bytes
SP_SWAR_HD uint32_t sp_swar_byte_count(uint64_t flags) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_popcountll(flags);
#else
    uint32_t n = 0;
    for (int q = 7; q < 64; q += 8) n += (uint32_t)(flags >> q & 1ULL);
    return n;
#endif
}
