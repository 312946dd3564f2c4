// sp_blocks.h -- the arithmetic of the homoeologous-block stage, compiled for the host and for the device.
//
// The reference obtains the collinear blocks of the innermost ring of its figure by running minimap2 / unimap on every
// pair of homoeologous chromosomes (Blocks.py:7-56: the pair list of run_align, chromosomes above 25 Mb cut into pieces)
// and keeping the primary alignments of alen >= -min_block (Circos.paf2blocks, Circos.py:654-682).  Here the packed
// genome is already resident, and blocks of 100 kb need no aligner: k-mers that occur exactly once in each of two
// chromosomes are anchors, and windows whose anchors vote for one diagonal are blocks.  Everything below is integers;
// tests/blocks_ref.py is the plain Python twin, written from the definition and compared with `==`.
//
//   k-mer      a start is valid when none of its kb bases is invalid (sp_bad_starts64); key = min(fwd, rc) in key order
//              (first base most significant, A = 0 .. T = 3), fw = (fwd < rc).  kb is odd: no palindromes.
//   sampling   a key is sampled when the low s bits of sp_bk_mix(key) are zero (s = 0: every key)
//   single     a sampled key with exactly one valid start in the chromosome: record (key, pos, fw)
//   anchor     of the ordered pair (A, B): a key single-copy in both: (posA, posB, opp = fwA != fwB)
//   vote       wa = posA / bin, wb = posB / bin; the call of an A-window is the cell (wb, opp) with the most anchors,
//              ties to opp = 0 before opp = 1, then to the smaller wb
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SP_BK_HD __host__ __device__
#else
#define SP_BK_HD
#endif

#define SP_BK_KMIN 17
#define SP_BK_KMAX 31
#define SP_BK_SMAX 16
#define SP_BK_MAXLEN 0x7ffffff0LL      // a position and its strand travel in 32 bits

// the splitmix64 finaliser
SP_BK_HD inline uint64_t sp_bk_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ULL;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return z;
}
SP_BK_HD inline bool sp_bk_sampled_mix(uint64_t mixed, int s) { return (mixed & ((1ULL << s) - 1ULL)) == 0; }
SP_BK_HD inline bool sp_bk_sampled(uint64_t key, int s) { return sp_bk_sampled_mix(sp_bk_mix(key), s); }

// home slot of a key in an index of `cap` entries (cap < 2^32): the HIGH half of the mix, the low s bits of which are
// zero for every key the index holds
SP_BK_HD inline uint32_t sp_bk_home(uint64_t mixed, uint32_t cap) { return (uint32_t)(((mixed >> 32) * (uint64_t)cap) >> 32); }

// parameters: 0 when good, else the number of the first bad one (1 = kb, 2 = s, 3 = bin)
SP_BK_HD inline int sp_bk_check(int kb, int s, int64_t bin) {
    if (kb < SP_BK_KMIN || kb > SP_BK_KMAX || !(kb & 1)) return 1;
    if (s < 0 || s > SP_BK_SMAX) return 2;
    if (bin < 1) return 3;
    return 0;
}
SP_BK_HD inline int64_t sp_bk_nwin(int64_t len, int64_t bin) { return (len + bin - 1) / bin; }

// A cell (wb, opp) as one number whose order is the tie order, and (count, cell) as one number whose MAXIMUM is the call:
// more anchors first, then the smaller cell.
SP_BK_HD inline uint32_t sp_bk_cell(int32_t wb, int opp) { return ((uint32_t)opp << 31) | (uint32_t)wb; }
SP_BK_HD inline uint64_t sp_bk_vote_pack(uint32_t count, uint32_t cell) { return ((uint64_t)count << 32) | (uint32_t)~cell; }
SP_BK_HD inline uint32_t sp_bk_vote_count(uint64_t v) { return (uint32_t)(v >> 32); }
SP_BK_HD inline int32_t sp_bk_vote_wb(uint64_t v) { return (int32_t)(~(uint32_t)v & 0x7fffffffu); }
SP_BK_HD inline int sp_bk_vote_opp(uint64_t v) { return (int)((~(uint32_t)v) >> 31); }

// the four outputs of one A-window from its best packed vote (0: no anchor) and its number of anchors
SP_BK_HD inline void sp_bk_vote_out(uint64_t best, int32_t total, int32_t *win_b, uint8_t *opp, int32_t *votes, int32_t *tot) {
    const bool any = sp_bk_vote_count(best) != 0;
    *win_b = any ? sp_bk_vote_wb(best) : -1;
    *opp = any ? (uint8_t)sp_bk_vote_opp(best) : (uint8_t)0;
    *votes = (int32_t)sp_bk_vote_count(best);
    *tot = total;
}
