"""Cases, inputs and staged references for the matcher's two path launches (csrc/sdr_paths.hip):
every k_paths / k_paths_tc / k_south_wta instantiation and the four k_sweep16 families, each
reached on purpose and named by the plan query.  Imports without a GPU; test_path_cases_cpu.py pins
the table and the references, test_gpu_path_cases.py runs it.

The instantiation a call takes depends on D (DPL 2 / 4 / 8 for D <= 128 / 256 / 512, PAD below the
class's 64 * DPL), the mode (NP = P - 1 directions read by the fused pass), the record format and
two chain-count thresholds in compute units.  The debug knob SDR_DEBUG_PLAN_CUS moves the thresholds:
KNOB_TC (1 CU) sends a frame of 24 columns to the two-chain / two-column kernels, KNOB_ONE (2^20
CUs) keeps any frame off them.
"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import numpy_ref as N
from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd._lib import SgbmParams
from test_oracle_sgm_volume import p2_domain_max

SGBM, HH, WAY3, HH4 = 0, 1, 2, 3
NP_OF = {WAY3: 2, HH4: 3, SGBM: 4, HH: 7}     # directions the fused pass reads: P - 1
MODE_OF = {v: k for k, v in NP_OF.items()}
KNOB_TC, KNOB_ONE = 1, 1 << 20
BS, P1, P2, UNIQ, D12, CAP = 3, 20, 120, 10, 1, 63
STAGE_ROWS = 384                               # kStageRows: one output staging window of k_south_wta

# record order of stage 4 as predecessor offsets (numpy_ref.SGM_DIRS' convention)
_E, _W, _S, _N, _SE, _SW, _NE, _NW = (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)
RECORDS = {WAY3: [_E, _W], HH4: [_E, _W, _N], SGBM: [_E, _W, _SE, _SW],
           HH: [_E, _W, _N, _SE, _SW, _NE, _NW]}


@dataclass(frozen=True)
class Case:
    name: str
    mode: int
    D: int
    H: int
    W1: int
    paths: tuple            # expected (family, DPL, PAD, R12) of the k_paths launch
    south: tuple            # expected ("k_south_wta", DPL, PAD, NP, TC, R12) or ("sweep", DW, PAD)
    knob: int = KNOB_ONE    # SDR_DEBUG_PLAN_CUS of the run (0: the device's own count)
    flip: int = 0           # the knob value of the second run on the same handle (0: none)
    minD: int = 0
    P2: int = P2
    uniq_rule: int = 1
    nstripes: int = 1
    F: int = 1
    kind: str = "band"      # "band": band_pair; "binary": synthetic.adversarial_pair
    seed: int = 1
    tiles: tuple = ()       # a sweep: expected (ntiles down, ntiles up)
    noise_every: int = 5    # band_pair's noise bands (3 at D = 16: see _build)
    bs: int = BS            # blockSize (the binary cases: 11, whose block costs alone pass 32767 / 8)
    tags: tuple = field(default=())

    @property
    def W(self):
        return self.W1 - min(self.minD, 0) + max(self.minD + self.D, 0)

    @property
    def minX1(self):
        return max(self.minD + self.D, 0)

    @property
    def args(self):
        return (self.minD, self.D, self.bs, P1, self.P2, D12, CAP, UNIQ, 0, 0, self.mode)

    @property
    def kwargs(self):
        return dict(nstripes=self.nstripes, uniq_rule=self.uniq_rule)

    def params(self):
        return SgbmParams(*self.args, self.nstripes, self.uniq_rule)

    def plan_key(self):
        """What sgbm_plan / last_plan must name for this case."""
        return self.paths, self.south


# ---- inputs ---------------------------------------------------------------------------------------

def band_shifts(nbands, D, seed):
    """Band k's disparity index: 0, D-1, 1, D-2, then seeded permutations of 0..D-1."""
    rng = np.random.default_rng(seed)
    d = [0, D - 1, 1, D - 2]
    while len(d) < nbands:
        d.extend(rng.permutation(D).tolist())
    return d[:nbands]


def band_pair(H, W1, D, seed, minD=0, noise_every=5):
    """A pair whose true disparity changes every 3 rows and visits the whole range.  The texture is
    random bytes smoothed [1 2 1]/4 along x; band k (rows 3k..3k+2) of the right image is the left
    texture shifted by d_k + minD, so left pixel x matches right pixel x - (d_k + minD); every 5th
    (noise_every-th)
    band of the right image is independent noise (no match: uniqueness rejections, LR conflicts),
    every 7th band is flat in both images (costs within the noise of each other: near-ties), and
    the whole right image then carries +-3 noise (non-zero subpixel terms)."""
    W = W1 - min(minD, 0) + max(minD + D, 0)
    rng = np.random.default_rng(seed)
    pad = D + abs(minD) + 8
    raw = rng.integers(0, 256, (H, W + 2 * pad + 2)).astype(np.int64)
    tex = (raw[:, :-2] + 2 * raw[:, 1:-1] + raw[:, 2:]) // 4
    left = tex[:, pad:pad + W].copy()
    right = np.empty_like(left)
    nb = (H + 2) // 3
    for k, dk in enumerate(band_shifts(nb, D, seed + 1)):
        ys = slice(3 * k, min(3 * k + 3, H))
        d = dk + minD  # right[x - d] = left[x]
        right[ys] = tex[ys, pad + d:pad + d + W]
        if k % noise_every == noise_every - 1:
            right[ys] = rng.integers(0, 256, right[ys].shape)
    for k in range(6, nb, 7):
        left[3 * k:3 * k + 3] = right[3 * k:3 * k + 3] = 128
    right = np.clip(right + rng.integers(-3, 4, right.shape), 0, 255)
    return left.astype(np.uint8), right.astype(np.uint8)


@lru_cache(maxsize=None)
def _pair(kind, H, W1, D, seed, minD, noise_every):
    if kind == "binary":
        W = W1 - min(minD, 0) + max(minD + D, 0)
        return S.adversarial_pair("binary", H, W, D, seed=seed)
    return band_pair(H, W1, D, seed, minD, noise_every)


def frames(c):
    """The case's F frames [(L, R), ...], each seeded differently."""
    return [_pair(c.kind, c.H, c.W1, c.D, c.seed + 101 * f, c.minD, c.noise_every) for f in range(c.F)]


# ---- the staged reference ---------------------------------------------------------------------------

def stripes(H, nstripes):
    """SGBM3WayMainLoop's (chain start, end, first output row) of every stripe."""
    sz = int(np.ceil(H / nstripes))
    overlap = (BS // 2 + 1) + int(np.ceil(0.1 * sz))
    return [(max(min(k * sz - overlap, H), 0), min((k + 1) * sz, H), k * sz)
            for k in range(nstripes) if k * sz < H]


def decode_rec12(raw, H, W1, nrec, D):
    """Stage 4's 12-bit records (sdr.h) as u32 words -> e = C - L [H][W1][nrec][D]."""
    w = raw.reshape(H, W1, nrec, D // 8, 3).astype(np.int64)
    e = np.empty((H, W1, nrec, D // 8, 8), np.int64)
    for j in range(3):
        e[..., 2 * j] = w[..., j] & 0xfff
        e[..., 2 * j + 1] = (w[..., j] >> 16) & 0xfff
    e[..., 6] = sum(((w[..., j] >> 12) & 0xf) << (4 * j) for j in range(3))
    e[..., 7] = sum(((w[..., j] >> 28) & 0xf) << (4 * j) for j in range(3))
    return e.reshape(H, W1, nrec, D)


@dataclass
class Staged:
    C: np.ndarray        # stage 0 [H][W1][D] int16
    recs: np.ndarray     # stage 4 as path costs [H][W1][R][D] int16 (a sweep: E, W, up)
    S: np.ndarray        # the saturated sums [H][W1][D] int64
    raw: np.ndarray      # stage 1 [H][W] int16 (INVALID outside the matched columns)
    keys: np.ndarray     # stage 5 [H][W] uint32
    lr: np.ndarray       # stage 2 [H][W] int16
    best: np.ndarray     # the winners' disparity index [H][W1]
    acc: np.ndarray      # accepted (unique, not saturated) [H][W1]
    eff: dict


def staged(L, R, c, sweep=False, segs=None):
    """Every stage of one frame from numpy_ref's restatement: the cost volume, each direction's L
    as its own volume (3WAY: per stripe, on the stripe's own cost rows), the saturated sum, the WTA
    map, the right view's keys and the LR verdict.  sweep: stage 4 as the batched MODE_HH sweep
    leaves it -- E, W and the up record min(32767, N + NE + NW).  segs: other (chain start, end,
    first output row) triples than the mode's own (a mutation's)."""
    e = N.sgm_effective(c.minD, c.D, c.bs, P1, c.P2, D12, CAP, UNIQ, c.mode, c.uniq_rule)
    H, W = L.shape
    minX1, W1 = c.minX1, c.W1
    pix = N.bt_cost_volume_rows(L, R, c.minD, c.D, e["ftzero"]).astype(np.int64)
    s = e["SW2"]
    xi = np.clip(np.arange(W1)[:, None] + np.arange(-s, s + 1)[None, :], 0, W1 - 1)
    hs = pix[:, xi, :].sum(2)
    hh = c.mode in (HH, HH4)
    Cmain = e["P2"] + N._box_rows(hs, 0, H, e["SH2"], hh)
    if segs is None:
        segs = stripes(H, c.nstripes) if c.mode == WAY3 else [(0, H, 0)]
    order = RECORDS[c.mode]
    if sweep:
        order = [_E, _W]
    recs = np.zeros((H, W1, 3 if sweep else len(order), c.D), np.int16)
    Ssum = np.zeros((H, W1, c.D), np.int64)
    assert Cmain.max() <= 32767
    for s0, end, out0 in segs:
        C = Cmain if (s0, end) == (0, H) else e["P2"] + N._box_rows(hs, s0, end, e["SH2"], hh)
        tot = np.zeros_like(C)
        up = np.zeros_like(C)
        for d in N.SGM_DIRS[c.mode]:
            Lv = N._path_volume(C, d[0], d[1], e["P1"], e["P2"])
            assert 0 <= Lv.min() and Lv.max() <= 32767
            tot += Lv
            if d in order:
                recs[out0:end, :, order.index(d)] = Lv[out0 - s0:]
            if d in (_N, _NE, _NW):
                up += Lv
        if sweep:
            recs[:, :, 2] = np.minimum(up, 32767)
        Ssum[out0:end] = np.minimum(tot, 32767)[out0 - s0:]
    d16, best, minS, acc = N.wta_map(Ssum, e)
    raw = np.full((H, W), (c.minD - 1) * 16, np.int64)
    raw[:, minX1:minX1 + W1] = d16
    keys = N.disp2_keys(best, minS, acc, e, W, minX1)
    lr = N.lr_verdict(raw, keys, e, minX1, W1)
    return Staged(Cmain.astype(np.int16), recs, Ssum, raw.astype(np.int16), keys,
                  lr.astype(np.int16), best, acc, e)


@lru_cache(maxsize=2)
def reference(c, f=0):
    """The staged reference of frame f of a case, computed once (the last few cases stay cached:
    a test uses one case, the natural-dispatch cases share their frames' references)."""
    L, R = frames(c)[f]
    return staged(L, R, c, sweep=c.south[0] == "sweep")


def chain_E(C, p1, p2, cut=0):
    """L of the left-to-right direction, rows in parallel: the recurrence restated in one dimension
    (cut = 0 equals numpy_ref._path_volume(C, 1, 0)).  cut > 0 is the mutation of a lane boundary
    gone wrong: disparity d with d % cut == 0 loses its d - 1 neighbour, d % cut == cut - 1 its
    d + 1 neighbour."""
    H, W1, D = C.shape
    C = C.astype(np.int64)
    L = np.empty_like(C)
    lp = np.zeros((H, D), np.int64)
    big = 1 << 40
    dd = np.arange(D)
    for x in range(W1):
        dn = np.concatenate([np.full((H, 1), big), lp[:, :-1]], 1)
        up = np.concatenate([lp[:, 1:], np.full((H, 1), big)], 1)
        if cut:
            dn = np.where(dd % cut == 0, big, dn)
            up = np.where(dd % cut == cut - 1, big, up)
        delta = lp.min(1, keepdims=True) + p2
        lp = C[:, x] + np.minimum(np.minimum(lp, np.minimum(dn, up) + p1), delta) - delta
        L[:, x] = lp
    return L


# ---- the table ------------------------------------------------------------------------------------

# (D, DPL, PAD): both ends of each padded class and the three full widths
D_CLASSES = [(16, 2, True), (112, 2, True), (128, 2, False), (144, 4, True), (240, 4, True),
             (256, 4, False), (272, 8, True), (496, 8, True), (512, 8, False)]
TALL, MID = 2 * STAGE_ROWS + 13, STAGE_ROWS + 13   # 781: a window's buffer reused; 397: one boundary
HEIGHTS = (1, 2, 11, 12, 13, 24, 25)               # chains shorter than a block; the PD, NS, window tails


def _south(dpl, pad, np_, tc=False, r12=False):
    return ("k_south_wta", dpl, pad, np_, tc, r12)


def _paths(dpl, pad, r12=False):
    return ("k_paths", dpl, pad, r12)


def _tc_paths(mode, pad):
    """Under KNOB_TC the E / W / N launches of 3WAY and HH4 take two chains a wave; MODE_SGBM's
    diagonals keep k_paths."""
    return ("k_paths_tc", 4, pad, False) if mode in (WAY3, HH4) else _paths(2, pad)


# Seeds other than a case's ordinal, where the ordinal's frame misses one of the input conditions
# (test_path_cases_cpu.py): the conditions hold as stated, the seed moves.
SEEDS = {"one-D144-np2": 1013, "one-D240-np2": 1017, "one-D240-np7": 1020, "one-D256-np7": 2024,
         "one-D272-np7": 1028, "one-D496-np2": 4029, "one-D512-np4": 1035, "one-D512-np7": 1036,
         "tc-D112-stripes-w24": 13047, "tc-D128-stripes-w25": 1051, "tc-D128-stripes-w24": 1055,
         "minD-5-one": 1084, "minD-5-r12": 2085, "minD-5-tc": 2086, "short-37-D496": 20093}


def _build():
    cases = []
    n = [0]

    def add(name, mode, D, H, W1, paths, south, **kw):
        n[0] += 1
        kw.setdefault("uniq_rule", 1 + n[0] % 2)  # the scalar and the SIMD rule in alternation
        kw.setdefault("seed", SEEDS.get(name, n[0]))
        if mode == WAY3:
            kw.setdefault("nstripes", 1)
        cases.append(Case(name, mode, D, H, W1, paths, south, **kw))

    # one column, int16 records: every DPL x PAD x NP.  D = 128 takes P2 = 4096 (past 12 bits: int16
    # records with no environment variable).  TALL for every DPL 2 form and for one NP of each wider
    # (DPL, PAD), at its first D -- a different NP each -- MID for the rest.  At D = 16 a random
    # winner among 16 candidates is mostly unique: the standard frame is accepted at 0.91 under
    # every seed (uniqueness rejects 0.09), so these cases' right images are noise in every 3rd band
    # instead of every 5th, and the input conditions stay as they are.
    tall = {(144, 2), (256, 3), (272, 4), (512, 7)}
    for D, dpl, pad in D_CLASSES:
        for np_ in (2, 3, 4, 7):
            mode = MODE_OF[np_]
            H = TALL if dpl == 2 or (D, np_) in tall else MID
            flip = KNOB_TC if dpl == 2 and np_ != 7 else 0
            add(f"one-D{D}-np{np_}", mode, D, H, 24, _paths(dpl, pad), _south(dpl, pad, np_),
                P2=4096 if D == 128 else P2, flip=flip, noise_every=3 if D == 16 else 5, tags=("one",))
    # 12-bit records (D = 128, P2 <= 4095): the benchmark's default kernels
    for np_ in (3, 4, 7):
        add(f"r12-np{np_}", MODE_OF[np_], 128, TALL, 24, _paths(2, False, True),
            _south(2, False, np_, r12=True), flip=KNOB_TC if np_ != 7 else 0, tags=("r12",))
    # two columns: PAD x NP 2, 3, 4 at an odd and an even W1; 3WAY as one stripe of TALL rows and as
    # four stripes of 37 (overlap rows recurred through and never output: kwrite)
    for D, pad in ((112, True), (128, False)):
        for W1 in (25, 24):
            for np_ in (2, 3, 4):
                mode = MODE_OF[np_]
                add(f"tc-D{D}-np{np_}-w{W1}", mode, D, TALL, W1, _tc_paths(mode, pad),
                    _south(2, pad, np_, tc=True), knob=KNOB_TC, flip=KNOB_ONE, tags=("tc",))
            add(f"tc-D{D}-stripes-w{W1}", WAY3, D, 37, W1, _tc_paths(WAY3, pad),
                _south(2, pad, 2, tc=True), knob=KNOB_TC, flip=KNOB_ONE, nstripes=4, tags=("tc", "stripes"))
    # heights: one instantiation per DPL and one two-column form
    for H in HEIGHTS:
        add(f"h{H}-D16", SGBM, 16, H, 24, _paths(2, True), _south(2, True, 4), tags=("height",))
        add(f"h{H}-D256", HH4, 256, H, 24, _paths(4, False), _south(4, False, 3), tags=("height",))
        add(f"h{H}-D272", HH, 272, H, 24, _paths(8, True), _south(8, True, 7), tags=("height",))
        add(f"h{H}-tc", SGBM, 16, H, 25, _paths(2, True), _south(2, True, 4, tc=True), knob=KNOB_TC,
            flip=KNOB_ONE, tags=("height", "tc"))
    # minDisparity -5 and +3 (the right view's column range), one case per family
    for minD in (-5, 3):
        add(f"minD{minD}-one", SGBM, 48, 37, 24, _paths(2, True), _south(2, True, 4), minD=minD, tags=("minD",))
        add(f"minD{minD}-r12", HH4, 128, 37, 24, _paths(2, False, True), _south(2, False, 3, r12=True),
            minD=minD, tags=("minD",))
        add(f"minD{minD}-tc", HH4, 48, 37, 25, _tc_paths(HH4, True), _south(2, True, 3, tc=True),
            knob=KNOB_TC, flip=KNOB_ONE, minD=minD, tags=("minD", "tc"))
        add(f"minD{minD}-sweep", HH, 48, 13, 41, ("k_paths", 2, True, False), ("sweep", 4, True), knob=0,
            minD=minD, F=8, tiles=(2, 1), tags=("minD", "sweep"))
    # short and wide: 13 rows of 130 columns, and 37 rows at D = 496
    add("wide-13x130-D48", SGBM, 48, 13, 130, _paths(2, True), _south(2, True, 4), tags=("wide",))
    add("short-37-D496", HH, 496, 37, 24, _paths(8, True), _south(8, True, 7), tags=("wide",))
    # every NP = 7 family on independent 0/255 pixels at the largest P2 of blockSize 11, where a
    # pixel's eight path costs pass 32767 at every disparity: saturated sums, pixels with no winner
    pmax = p2_domain_max(11, CAP, HH)
    for D, dpl, pad in ((112, 2, True), (128, 2, False), (240, 4, True), (256, 4, False), (496, 8, True),
                        (512, 8, False)):
        add(f"binary-D{D}", HH, D, 25, 24, _paths(dpl, pad), _south(dpl, pad, 7), P2=pmax, kind="binary",
            bs=11, tags=("binary",))
    add("binary-r12", HH, 128, 25, 24, _paths(2, False, True), _south(2, False, 7, r12=True), P2=4095,
        kind="binary", bs=11, tags=("binary",))
    # batched MODE_HH: the four sweep families (DW x PAD) at one tile of both passes, at one column
    # past the down pass's tile (40 columns) and one past the up pass's (80); D = 272 takes chains
    for D, dw, pad in ((16, 4, True), (128, 4, False), (144, 8, True), (256, 8, False)):
        dpl = 2 if D <= 128 else 4
        for W1, tiles in ((40, (1, 1)), (41, (2, 1)), (81, (3, 2))):
            add(f"sweep-D{D}-w{W1}", HH, D, 13, W1, _paths(dpl, pad), ("sweep", dw, pad), knob=0, F=8,
                tiles=tiles, tags=("sweep",))
    add("sweep-D272-chains", HH, 272, 13, 24, _paths(8, True), _south(8, True, 7), knob=0, F=8,
        tags=("batch",))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def natural_cases(cus):
    """No knob: MODE_SGBM and MODE_HH4 batches of F frames whose W1 * F column chains sit just above
    8 * cus (two columns) and, one frame smaller, below it (one column), at D = 16 and D = 128.
    The paths launch follows the same count at 4 * cus for MODE_HH4's 2H + W1 chains a frame."""
    out = []
    F, H = 8, 25
    W1 = 8 * cus // F + 1
    for D, pad in ((16, True), (128, False)):
        for mode in (SGBM, HH4):
            np_ = NP_OF[mode]
            for f in (F, F - 1):
                tc = W1 * f > 8 * cus
                tcp = mode == HH4 and (2 * H + W1) * f > 4 * cus
                r12 = D == 128 and not tc and not tcp
                paths = ("k_paths_tc", 4, pad, False) if tcp else _paths(2, pad, r12)
                out.append(Case(f"natural-D{D}-np{np_}-F{f}", mode, D, H, W1, paths,
                                _south(2, pad, np_, tc=tc, r12=r12), knob=0, F=f, seed=900 + D + mode,
                                uniq_rule=1 + (mode == HH4), tags=("natural",)))
    return out


# The full enumeration of the kernels the two launches can take (csrc/sdr_paths.hip, sdr_sweep.hip).
ALL_PATHS = {("k_paths", d, p, False) for d in (2, 4, 8) for p in (True, False)} | \
            {("k_paths", 2, False, True), ("k_paths_tc", 4, True, False), ("k_paths_tc", 4, False, False)}
ALL_SOUTH = {("k_south_wta", d, p, n, False, False) for d in (2, 4, 8) for p in (True, False) for n in (2, 3, 4, 7)} | \
            {("k_south_wta", 2, p, n, True, False) for p in (True, False) for n in (2, 3, 4)} | \
            {("k_south_wta", 2, False, n, False, True) for n in (3, 4, 7)}
ALL_SWEEPS = {("sweep", dw, p) for dw in (4, 8) for p in (True, False)}
assert (len(ALL_PATHS), len(ALL_SOUTH), len(ALL_SWEEPS)) == (9, 33, 4)
