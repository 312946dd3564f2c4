"""Plain Python twin of the homoeologous-block stage, written from the definition (not from csrc/sp_blocks.h):

  k-mer     a start is valid when none of its kb bases is anything but ACGT in either case; key = min(fwd, rc) with the
            first base most significant and A = 0, C = 1, G = 2, T = 3; fw = (fwd < rc); kb is odd
  sampling  a key is sampled when the low s bits of the splitmix64 finaliser of the key are zero
  single    a sampled key with exactly one valid start in the chromosome: (key, pos, fw)
  anchor    of the ordered pair (A, B): a key single-copy in both, (posA, posB, opp = fwA != fwB), ascending posA
  vote      wa = posA // bin, wb = posB // bin; per A-window the cell (wb, opp) with the most anchors, ties to opp = 0
            before opp = 1, then to the smaller wb; win_b = -1 when the window has no anchor
  blocks    the walk over called windows (votes >= min_votes) described at blocks()

Everything is integers and dictionaries; the device and subphaser_amd/blocks.py are compared with `==`."""
import numpy as np

M64 = (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}


def mix(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & M64
    z ^= z >> 31
    return z


def sampled(key, s):
    return mix(key) & ((1 << s) - 1) == 0


def check_params(kb, s, bin_size):
    if not (17 <= kb <= 31 and kb % 2 == 1):
        raise ValueError("kb")
    if not 0 <= s <= 16:
        raise ValueError("s")
    if bin_size < 1:
        raise ValueError("bin")


def kmers(seq, kb):
    """(pos, key, fw) of every valid start, ascending pos"""
    if isinstance(seq, bytes):
        seq = seq.decode()
    out = []
    fwd = rc = 0
    run = 0
    mask = (1 << (2 * kb)) - 1
    for i, ch in enumerate(seq):
        c = CODE.get(ch)
        if c is None:
            run = 0
            fwd = rc = 0
            continue
        fwd = ((fwd << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * (kb - 1)))
        run += 1
        if run >= kb:
            out.append((i - kb + 1, min(fwd, rc), fwd < rc))
    return out


def index(seq, kb, s):
    """{key: (pos, fw)} of the sampled single-copy keys, and (n_sampled, n_single)"""
    seen = {}
    n_sampled = 0
    for pos, key, fw in kmers(seq, kb):
        if not sampled(key, s):
            continue
        n_sampled += 1
        seen[key] = None if key in seen else (pos, fw)
    single = {k: v for k, v in seen.items() if v is not None}
    return single, (n_sampled, len(single))


def anchors(ia, ib):
    """[(posA, posB, opp)] ascending posA from two index() dictionaries"""
    out = [(pa, ib[key][0], int(fa != ib[key][1])) for key, (pa, fa) in ia.items() if key in ib]
    out.sort()
    return out


def vote(anch, len_a, bin_size):
    """win_b int32, opp uint8, votes int32, total int32 over the ceil(len_a / bin) windows of A"""
    n_win = -(-len_a // bin_size)
    win_b, opp = np.full(n_win, -1, np.int32), np.zeros(n_win, np.uint8)
    votes, total = np.zeros(n_win, np.int32), np.zeros(n_win, np.int32)
    cells = {}
    for pa, pb, o in anch:
        d = cells.setdefault(pa // bin_size, {})
        d[(pb // bin_size, o)] = d.get((pb // bin_size, o), 0) + 1
    for wa, d in cells.items():
        win_b[wa], opp[wa], votes[wa], total[wa] = vote_cells(d)
    return win_b, opp, votes, total


def vote_cells(d):
    """(win_b, opp, votes, total) of one window from {(wb, opp): count}"""
    if not d:
        return -1, 0, 0, 0
    (wb, o), n = min(d.items(), key=lambda kv: (-kv[1], kv[0][1], kv[0][0]))
    return wb, o, n, sum(d.values())


def pair(seq_a, seq_b, kb, s, bin_size):
    """everything the device reports for the ordered pair: (anchors, win_b, opp, votes, total)"""
    check_params(kb, s, bin_size)
    ia, _ = index(seq_a, kb, s)
    ib, _ = index(seq_b, kb, s)
    anch = anchors(ia, ib)
    return (anch,) + vote(anch, len(seq_a), bin_size)


def blocks(win_b, opp, votes, len_a, len_b, bin_size, min_votes, max_gap, min_block):
    """The walk: A-windows with votes >= min_votes in ascending wa; a window joins the open block when it has the same
    opp, dA = wa - wa_last <= max_gap + 1 and |dB - dA| <= max_gap, dB = wb - wb_last for opp = 0 and wb_last - wb for
    opp = 1; otherwise the block closes and the window opens a new one.  A block is (start1, end1, start2, end2, strand,
    windows, sum of votes), kept when end1 - start1 >= min_block."""
    out = []
    cur = None      # [wa_first, wa_last, wb_last, wb_min, wb_max, opp, windows, votes]

    def close():
        if cur is None:
            return
        s1, e1 = cur[0] * bin_size, min((cur[1] + 1) * bin_size, len_a)
        s2, e2 = cur[3] * bin_size, min((cur[4] + 1) * bin_size, len_b)
        if e1 - s1 >= min_block:
            out.append((s1, e1, s2, e2, "-" if cur[5] else "+", cur[6], cur[7]))

    for wa in range(len(win_b)):
        v, wb, o = int(votes[wa]), int(win_b[wa]), int(opp[wa])
        if v < min_votes or wb < 0:
            continue
        if cur is not None and o == cur[5]:
            dA = wa - cur[1]
            dB = cur[2] - wb if o else wb - cur[2]
            if dA <= max_gap + 1 and abs(dB - dA) <= max_gap:
                cur[1], cur[2] = wa, wb
                cur[3], cur[4] = min(cur[3], wb), max(cur[4], wb)
                cur[6] += 1
                cur[7] += v
                continue
        close()
        cur = [wa, wa, wb, wb, wb, o, 1, v]
    close()
    return out


# ---- brute force, independent of the 2-bit key code: Python strings only
_COMP = str.maketrans("ACGT", "TGCA")


def brute_anchors(seq_a, seq_b, kb, s):
    """anchors from string slicing and str reverse complement; the sampling decision still needs the number of the
    canonical string (the smaller of the two in A < C < G < T order, which is the order of the keys)"""
    def occurrences(seq):
        up = seq.upper()
        occ = {}
        for i in range(len(up) - kb + 1):
            w = up[i:i + kb]
            if set(w) - set("ACGT"):
                continue
            r = w.translate(_COMP)[::-1]
            occ.setdefault(min(w, r), []).append((i, w < r))
        return occ

    def number(w):
        n = 0
        for ch in w:
            n = n * 4 + "ACGT".index(ch)
        return n
    oa, ob = occurrences(seq_a), occurrences(seq_b)
    out = []
    for w, la in oa.items():
        lb = ob.get(w)
        if lb is None or len(la) != 1 or len(lb) != 1 or not sampled(number(w), s):
            continue
        out.append((la[0][0], lb[0][0], int(la[0][1] != lb[0][1])))
    out.sort()
    return out
