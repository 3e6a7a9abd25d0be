"""Inputs, input checks and runners shared by the FGS / WLS GPU parity tests (test_gpu_wls.py,
test_gpu_fgs_dispatch.py, its child processes fgs_dispatch_child.py) and the CPU check of the
generator (test_fgs_dispatch_cpu.py).  Nothing here needs a GPU until a run_* function is called.

The sequential solver (SDR_FGS_THOMAS) divides in two forms: from the pivot's reciprocal
(Markstein) in a 16-sample group, and with IEEE divisions where the reciprocal form is not
covered.  The coefficient jobs take the IEEE form in a group holding a tiny non-zero weight term
cc = lambda * C, 0 < |cc| < 2^-96 (1 + 2 lambda) (k_fgs_th's jobs: in a whole chunk); the passes
redo a group (k_fgs_th: a chunk) whose right-hand-side quotient came out 0 < |q| < 2^-96 and start
one in the IEEE form when the value entering it is below 2^-64.  structured_guide / structured_rhs
build inputs that reach both forms next to each other, at known samples; tiny_condition_errors
checks, from the oracle's weight table alone, that a guide does.
"""
import numpy as np

from stereo_depth_ruler_amd import synthetic as S
from stereo_depth_ruler_amd._lib import FGS_THOMAS, WlsParams, fgs_plan

PARAMS = [(8000.0, 1.1), (50.0, 5.0)]  # (lambda, sigma_color): the reference's, and a mild pair
BLOCK = 64  # the period of the guide's pattern: the shortest chunk of k_fgs_lr / k_fgs_lrjob (L = 16)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def wls_from_oracle_params(q) -> WlsParams:
    """The engine's parameters for exactly the oracle's (ROI given as offsets)."""
    return WlsParams(q.lambda_, q.sigma_color, q.lrc_thresh, q.depth_disc_radius, q.roll_off,
                     q.lambda_attenuation, q.num_iter, q.roi_x, 0, q.roi_y, 0, q.min_disp, q.fgs_solver)


def make_filter(q, W, H):
    from stereo_depth_ruler_amd.ximgproc import DisparityWLSFilter

    p = wls_from_oracle_params(q)
    p.right_offset = W - q.roi_x - q.roi_w
    p.bottom_offset = H - q.roi_y - q.roi_h
    return DisparityWLSFilter(p)


def sgbm_pair_maps(oracle, h, w, numD, seed, minD=0):
    """Left / right disparity maps produced by the oracle SGBM on a synthetic pair, the way the
    class path produces them (left matcher WLS-mutated, right matcher from createRightMatcher)."""
    L, R, _ = S.make_pair(h, w, numD, seed=seed)
    dl = oracle.sgbm_compute(L, R, oracle.make_params(minD, numD, 5, 600, 2400, 1000000, 63, 0, 0, 2, 2))
    dr = oracle.sgbm_compute(R, L, oracle.make_params(-(minD + numD) + 1, numD, 5, 600, 2400, 1000000,
                                                      63, 0, 0, 2, 2))
    return L, dl, dr


def hyp_case(oracle, rng, W, H, guide, lam, sigma, D=80):
    """A WLS input of the verdict's hypothesis space: flat, binary-edge, noise
    or scene guides, or a given (H, W) uint8 guide; block-constant disparities with 10 % invalid
    pixels (a sparse confidence map) for all but `scene`, which takes the matcher pair of a
    synthetic frame.  D = numDisparities (minDisparity 0): the ROI is W - D wide."""
    if isinstance(guide, str) and guide == "scene":
        L, dl, dr = sgbm_pair_maps(oracle, H, W, D, int(rng.integers(1 << 30)))
        g = L
    else:
        if not isinstance(guide, str):
            g = np.ascontiguousarray(guide, np.uint8)
            assert g.shape == (H, W)
        elif guide == "flat":
            g = np.full((H, W), int(rng.integers(0, 256)), np.uint8)
        elif guide == "edge":
            g = np.zeros((H, W), np.uint8)
            g[:, int(rng.integers(1, W)):] = 255
            g[int(rng.integers(1, H)):, :] ^= 255
        else:
            g = rng.integers(0, 256, (H, W), dtype=np.uint8)
        blocks = rng.integers(0, D * 16, ((H + 7) // 8, (W + 7) // 8))
        dl = np.repeat(np.repeat(blocks, 8, 0), 8, 1)[:H, :W].astype(np.int16)
        dl[rng.random((H, W)) < 0.1] = -16
        dr = -np.clip(dl, 0, None).astype(np.int16)
    q = oracle.wls_params_for_sgbm(0, D, 5, W, H, lam, sigma)
    return g, dl, dr, q


# ---- structured inputs ---------------------------------------------------------------------

def _quiet(n, quiet_every):
    """The samples of the quiet blocks: block b with b % quiet_every == quiet_every - 1."""
    k = np.arange(n)
    return (k // BLOCK) % quiet_every == quiet_every - 1 if quiet_every else np.zeros(n, bool)


def _toggles(n, quiet_every):
    """The samples k whose weight (between k and k + 1) is an isolated step: in every block of 64
    samples the first group (k = 3), the last (59, 62), the block boundary itself (63) and the next
    block's first weight (64); and the line's last weight when its last group holds one.  A block
    b with b % quiet_every == quiet_every - 1 holds none (quiet_every = 0: every block has them)."""
    t = {k for k in range(n - 1) if k % BLOCK in (3, 59, 62, 63) or (k % BLOCK == 0 and k > 0)}
    if quiet_every:
        t = {k for k in t if (k // BLOCK) % quiet_every != quiet_every - 1}
    if n >= 2 and n - 2 >= 16 * ((n - 1) // 16):
        t.add(n - 2)
    return t


def _profile(rng, n, quiet_every):
    """One axis of the guide: a ramp with steps <= 3 inside [0, 15], lifted by 84..108 gray levels
    between every other pair of toggles, so that the difference across a toggle is 81..111 (a
    weight that is tiny but not zero at sigma 1.1) and at most 3 everywhere else."""
    steps = rng.integers(-3, 4, n)
    r = np.empty(n, np.int64)
    v = int(rng.integers(0, 16))
    tog = _toggles(n, quiet_every)
    high, off = False, 0
    for k in range(n):
        v = min(15, max(0, v + int(steps[k])))
        r[k] = v + (off if high else 0)
        if k in tog:
            high = not high
            off = int(rng.integers(84, 109))
    return r


def _band(n):
    """The lines that carry the other axis's 0/255 edges and small runs: where a line is long enough
    to have chunks, only samples of a block's last group (so that what they do to the weights
    along this axis stays inside a group that holds a step anyway); every 4th where it is not."""
    k = np.arange(n)
    return (k % BLOCK >= 52) & (k % BLOCK < 60) if n >= 32 else k % 4 == 1


def structured_guide(rng, h, w, quiet_rows=0, quiet_cols=0):
    """An (h, w) guide of smooth ramps, isolated steps of 81..111 gray levels at known samples of
    every line, both ways (see _toggles), and 0/255 edges (weight exactly zero) at samples 50 | 51
    of a block on the lines of _band.  quiet_rows / quiet_cols: every so-many-th block along the
    rows / the columns holds no step (for k_fgs_th's jobs, which flag whole chunks)."""
    g = _profile(rng, w, quiet_rows)[None, :] + _profile(rng, h, quiet_cols)[:, None]
    assert g.max() <= 255
    g = g.astype(np.uint8)
    # (a quiet block holds no edge either, and none of the other axis's edge lines: the differences
    # next to an edge are whatever the ramps leave, tiny on some lines)
    qw, qh = _quiet(w, quiet_rows), _quiet(h, quiet_cols)
    rows, cols = _band(h) & ~qh, _band(w) & ~qw
    for j in range(50, w - 1, BLOCK):
        if not qw[j]:
            g[rows, j], g[rows, j + 1] = 0, 255
    for i in range(50, h - 1, BLOCK):
        if not qh[i]:
            g[i, cols], g[i + 1, cols] = 0, 255
    return g


def structured_rhs(rng, h, w):
    """Right-hand sides of normal values, blocks of exact zeros (samples 4..43 of every other block,
    right behind a step, on half of the lines: the elimination then carries a * u ~ 2^-90 and
    smaller through them) and runs of magnitudes near 2^-70 behind the 0/255 edges (samples
    51..69 of a block, across a group's and a block's start, on the lines of _band); zero on the
    isolated cells (isolated_cells)."""
    x = (rng.random((h, w)) * 1000).astype(np.float32)
    i, j = np.arange(h), np.arange(w)
    zr = (j % BLOCK >= 4) & (j % BLOCK < 44) & ((j // BLOCK) % 2 == 1)
    zc = (i % BLOCK >= 4) & (i % BLOCK < 44) & ((i // BLOCK) % 2 == 1)
    x[(zr[None, :] & ((i // 4) % 2 == 0)[:, None]) | (zc[:, None] & ((j // 4) % 2 == 1)[None, :])] = 0.0
    small = (np.float32(2.0 ** -70) * (1 + rng.random((h, w))) * rng.choice([-1.0, 1.0], (h, w))).astype(np.float32)
    sr = (j >= 51) & ((j - 51) % BLOCK < 19)
    sc = (i >= 51) & ((i - 51) % BLOCK < 19)
    m = (sr[None, :] & _band(h)[:, None]) | (sc[:, None] & _band(w)[None, :])
    x[m] = small[m]
    x[isolated_cells(h, w)] = 0.0
    return x


def isolated_cells(h, w):
    """The samples that steps cut off from the rest of the image both ways: the last three samples
    and the boundary sample of a block and the first four of the next (60..63 | 0..3, between the
    steps at 59 and at 3), along the rows AND along the columns.  With a zero right-hand side there,
    the solution inside is what leaks through the steps, t * u of the neighbour with t = cc / den
    tiny or subnormal: the one place where a coefficient job's quotient in the wrong division form
    (an ulp of a subnormal t) reaches the output's bits instead of vanishing under normal values."""
    i, j = np.arange(h), np.arange(w)
    return (((i + 4) % BLOCK) < 8)[:, None] & (((j + 4) % BLOCK) < 8)[None, :]


def lambdas(lam, att=0.25, iters=3):
    """The passes' lambdas in the filter's float arithmetic (lambda *= attenuation)."""
    out, v = [], np.float32(lam)
    for _ in range(iters):
        out.append(v)
        v = np.float32(v * np.float32(att))
    return out


def tiny_weights(oracle, g, lam, sigma):
    """Per direction, where a weight term cc = lambda * C of the guide is tiny but not zero,
    0 < |cc| < 2^-96 (1 + 2 lambda), for EVERY pass's lambda: (rows (h, w), cols (h, w)) booleans,
    element [i, j] for the weight between (i, j) and its right / lower neighbour.  From the
    oracle's table alone."""
    lut = oracle.fgs_lut(sigma)
    gi = g.astype(np.int64)
    h, w = g.shape
    Ch = np.zeros((h, w), np.float32)
    Cv = np.zeros((h, w), np.float32)
    Ch[:, :-1] = lut[(gi[:, :-1] - gi[:, 1:]) ** 2]
    Cv[:-1, :] = lut[(gi[:-1, :] - gi[1:, :]) ** 2]
    out = []
    for C in (Ch, Cv):
        t = np.ones((h, w), bool)
        for l in lambdas(lam):
            cc = np.abs(l * C)  # float32, as the jobs compute it
            t &= (cc > 0) & (cc < np.float32(2.0 ** -96) * (np.float32(1) + np.float32(2) * l))
        out.append(t)
    return out


def _axis_errors(t, kernel, lines, what):
    """t: (nlines, n) tiny flags of the lines along one axis.  k_fgs_lr / k_fgs_lrjob (the IEEE form
    per 16-sample group): every chunk (1024 / lines samples) of at least three groups holds a group
    with a tiny weight and a group without (a chunk of two groups is its first and its last group,
    where the steps sit by construction).  k_fgs_th (per chunk): every line of at least 256 samples
    holds a chunk with and a chunk without."""
    nl, n = t.shape
    ng = (n + 15) // 16
    grp = np.zeros((nl, ng * 16), bool)
    grp[:, :n] = t
    grp = grp.reshape(nl, ng, 16).any(2)  # (line, group): holds a tiny weight
    errs = []
    ch = 1024 // lines // 16  # groups a chunk
    if kernel == "th":
        if n < 256:
            return errs
        nch = (ng + ch - 1) // ch
        pad = np.zeros((nl, nch * ch), bool)
        pad[:, :ng] = grp
        chunk = pad.reshape(nl, nch, ch).any(2)
        bad = ~(chunk.any(1) & (~chunk).any(1))
        if bad.any():
            errs.append(f"{what}: {int(bad.sum())} line(s) without both a tiny and a clean chunk of {ch * 16}")
        return errs
    for c0 in range(0, ng, ch):
        c1 = min(c0 + ch, ng)
        if min(c1 * 16, n) - c0 * 16 < 48:
            continue
        sub = grp[:, c0:c1]
        bad = ~(sub.any(1) & (~sub).any(1))
        if bad.any():
            errs.append(f"{what}: chunk at sample {c0 * 16}: {int(bad.sum())} line(s) without both a "
                        "tiny and a clean group")
    return errs


def tiny_condition_errors(oracle, g, lam, sigma, plan):
    """The input condition of the dispatch tests for guide g (the FGS image or the WLS ROI) under
    `plan` (fgs_plan's dict): [] when every chunk of every line, rows and columns, for the pass's
    and the job's chunk length, meets _axis_errors' condition."""
    tr, tc = tiny_weights(oracle, g, lam, sigma)
    errs = []
    for t, axis in ((tr, "row"), (tc.T, "col")):
        for role in ("pass", "job"):
            kernel, lines = plan[f"{axis}_{role}"]
            errs += _axis_errors(t, kernel, lines, f"{axis} {role} ({kernel}, {lines})")
    return errs


def quiet_for(plan):
    """structured_guide's quiet_rows / quiet_cols for a plan: 4 where k_fgs_th computes the axis's
    coefficients (it flags whole chunks), 0 elsewhere."""
    return (4 if plan["row_job"][0] == "th" else 0, 4 if plan["col_job"][0] == "th" else 0)


def no_tiny_weight_possible(oracle, lam, sigma):
    """True when no difference of two 8-bit gray levels gives a tiny non-zero weight term at any
    pass's lambda: every group of every job then takes the reciprocal form."""
    lut = oracle.fgs_lut(sigma)[np.arange(256) ** 2]
    for l in lambdas(lam):
        cc = np.abs(l * lut)
        if ((cc > 0) & (cc < np.float32(2.0 ** -96) * (np.float32(1) + np.float32(2) * l))).any():
            return False
    return True


def check_inputs(oracle, g, lam, sigma, plan):
    """A condition on the inputs, from the reference alone: at (8000, 1.1) the guide reaches both
    division forms in every chunk (tiny_condition_errors); at (50, 5.0) no 8-bit step is tiny, so
    every group takes the reciprocal form."""
    if no_tiny_weight_possible(oracle, lam, sigma):
        return []
    return tiny_condition_errors(oracle, g, lam, sigma, plan)




# ---- runners: [] or a list of what went wrong ------------------------------------------------
# A case is a JSON-able dict: {"entry": "fgs" | "wls", "h", "w" (fgs: the image; wls: the ROI, the
# map is 16 columns wider), "nimg" (fgs: the stack), "expect": {fgs_plan key: [family, lines]}};
# lines None: whatever the query says (k_fgs_th's lines depend on the device's compute units).

def plan_errors(plan, expect):
    return [f"plan {k} = {plan[k]}, expected {tuple(v)}" for k, v in expect.items()
            if plan[k][0] != v[0] or (v[1] is not None and plan[k][1] != v[1])]


def seed_of(*a):
    return int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(a)) % (1 << 31))


def run_fgs(oracle, h, w, nimg, expect, cus=0, inputs_only=False, params=PARAMS):
    """fastGlobalSmootherFilter on a stack of nimg structured images (solved in pairs, a left-over
    image alone) against the oracle, bit for bit, after asserting the plan of the stack's first
    launch and the condition on the inputs.  inputs_only: stop before the device call."""
    plan = fgs_plan(w, h, 1, min(nimg, 2), cus=cus)
    errs = plan_errors(plan, expect)
    if errs:
        return errs
    rng = np.random.default_rng(seed_of(h, w, nimg))
    g = structured_guide(rng, h, w, *quiet_for(plan))
    xs = np.stack([structured_rhs(rng, h, w) for _ in range(nimg)])
    for lam, sigma in params:
        errs += check_inputs(oracle, g, lam, sigma, plan)
        if errs or inputs_only:
            continue
        from stereo_depth_ruler_amd.ximgproc import fastGlobalSmootherFilter

        got = fastGlobalSmootherFilter(g, xs if nimg > 1 else xs[0], lam, sigma)
        got = got if nimg > 1 else got[None]
        for i in range(nimg):
            ref = oracle.fgs_filter(g, xs[i], lam, sigma)
            bad = bits(got[i]) != bits(ref)
            if bad.any():
                errs.append(f"fgs ({h}, {w}) image {i} of {nimg}, lambda {lam} sigma {sigma}: {int(bad.sum())} "
                            f"value(s) differ, first at {tuple(int(v) for v in np.argwhere(bad)[0])}")
    return errs


def wls_inputs(oracle, H, rw, lam, sigma, plan, seed=0):
    """A WLS case whose ROI is rw x H: numDisparities 16, minDisparity 0 (a map 16 columns wider),
    the structured guide over the ROI, hyp_case's block-constant disparities."""
    rng = np.random.default_rng(seed_of(H, rw, 3, seed))
    W = rw + 16
    g = np.empty((H, W), np.uint8)
    g[:, :16] = rng.integers(0, 256, (H, 16), dtype=np.uint8)
    g[:, 16:] = structured_guide(rng, H, rw, *quiet_for(plan))
    g, dl, dr, q = hyp_case(oracle, rng, W, H, g, lam, sigma, D=16)
    assert (q.roi_x, q.roi_y, q.roi_w, q.roi_h) == (16, 0, rw, H) and q.fgs_solver == FGS_THOMAS
    # zero confidence (both right-hand sides zero) on the ROI's isolated cells: a left disparity
    # of 15 px whose right-view partner, 15 columns to the left, holds 0 fails the LR check
    ii, jj = np.nonzero(isolated_cells(H, rw))
    dl[ii, jj + 16] = 240
    dr[ii, jj + 1] = 0
    return g, dl, dr, q


def run_wls(oracle, H, rw, expect, cus=0, inputs_only=False, params=PARAMS):
    """DisparityWLSFilter.filter on a map whose ROI is rw x H against the oracle: the filtered
    map and the confidence map, bit for bit, after the plan and input assertions."""
    plan = fgs_plan(rw, H, 1, 2, cus=cus)
    errs = plan_errors(plan, expect)
    if errs:
        return errs
    for lam, sigma in params:
        g, dl, dr, q = wls_inputs(oracle, H, rw, lam, sigma, plan)
        errs += check_inputs(oracle, g[:, 16:], lam, sigma, plan)
        if errs or inputs_only:
            continue
        ref, ref_conf = oracle.wls_filter(dl, dr, g, q, return_conf=True)
        f = make_filter(q, rw + 16, H)
        got = f.filter(dl, g, dr)
        if not np.array_equal(bits(f.getConfidenceMap()), bits(ref_conf)):
            errs.append(f"wls ROI ({H}, {rw}), lambda {lam} sigma {sigma}: the confidence map differs")
        if not np.array_equal(got, ref):
            errs.append(f"wls ROI ({H}, {rw}), lambda {lam} sigma {sigma}: {int((got != ref).sum())} pixel(s) differ")
    return errs


def run_case(oracle, case, cus=0, inputs_only=False):
    if case["entry"] == "fgs":
        return run_fgs(oracle, case["h"], case["w"], case.get("nimg", 2), case["expect"], cus, inputs_only)
    return run_wls(oracle, case["h"], case["w"], case["expect"], cus, inputs_only)


def case_id(c):
    return f"{c['name']}-{c['h']}x{c['w']}-{c['entry']}" + (f"{c['nimg']}" if c.get("nimg", 2) != 2 else "")


# ---- the cases -------------------------------------------------------------------------------
# Lines of n samples, m of them, as rows (an (m, n) image) and as columns ((n, m)); m below, at,
# one past and several past the lines a workgroup.

def _line_cases(name, table, along, across, entries=("fgs", "wls"), nimg=2):
    """along / across: {"pass": [family, lines], "job": [family, lines]} of the axis of the long
    lines / of the short ones."""
    out = []
    for n, ms in table.items():
        for m in ms:
            for orient in ("rows", "cols"):
                a, b = ("row", "col") if orient == "rows" else ("col", "row")
                expect = {f"{a}_pass": along["pass"], f"{a}_job": along["job"],
                          f"{b}_pass": across["pass"], f"{b}_job": across["job"]}
                h, w = (m, n) if orient == "rows" else (n, m)
                for e in entries:
                    out.append({"name": f"{name}-{orient}", "entry": e, "h": h, "w": w, "nimg": nimg,
                                "expect": expect})
    return out


# the short axis (m <= 40 samples): k_fgs_lr at the default cap of 8 lines, its job on 16
_SHORT = {"pass": ["lr", 8], "job": ["lrjob", 16]}
_SHORT_TH = {"pass": ["lr", 8], "job": ["th", None]}  # (one job past 1536 samples: all on k_fgs_th)

LR4 = _line_cases("lr4", {769: (1, 4, 9), 1024: (3, 5), 1025: (4, 24), 1100: (1, 5, 9), 1535: (3, 4),
                          1536: (5, 24)}, {"pass": ["lr", 4], "job": ["lrjob", 4]}, _SHORT)
LR2 = _line_cases("lr2", {1537: (1, 3, 9), 2048: (1, 4), 2049: (3, 24), 2100: (5, 9), 3071: (1, 3),
                          3072: (4, 24)}, {"pass": ["lr", 2], "job": ["th", None]}, _SHORT_TH)
TH_PAST = _line_cases("th16", {3073: (1, 5, 24)}, {"pass": ["th", 16], "job": ["th", None]}, _SHORT_TH)
LR8 = _line_cases("lr8", {385: (5, 9), 767: (3, 9, 24), 768: (1, 9, 24)},
                  {"pass": ["lr", 8], "job": ["lrjob", 8]}, _SHORT)
# a stack of 3: one pair and a single image (k_fgs_th<false, 16> passes, the same jobs)
STACK3 = [{"name": "stack3", "entry": "fgs", "h": 5, "w": 1100, "nimg": 3,
           "expect": {"row_pass": ["lr", 4], "row_job": ["lrjob", 4], "col_pass": ["lr", 8],
                      "col_job": ["lrjob", 16]}}]


def _job_lines(n):
    return 16 if n <= 384 else 8 if n <= 768 else 4


def _mixed():
    """All nine (row job L, column job L) pairs in one k_fgs_lrjob launch; then a job past 1536
    samples, which sends every job of the launch to k_fgs_th."""
    out = []
    for h in (20, 400, 800):
        for w in (24, 420, 900):
            lw, lh = _job_lines(w), _job_lines(h)
            expect = {"row_job": ["lrjob", lw], "col_job": ["lrjob", lh],
                      "row_pass": ["lr", min(lw, 8)], "col_pass": ["lr", min(lh, 8)]}
            for e in ("fgs", "wls"):
                out.append({"name": f"jobs{lw}x{lh}", "entry": e, "h": h, "w": w, "nimg": 2, "expect": expect})
    for (h, w), cp in (((800, 1600), 4), ((24, 1600), 8)):
        expect = {"row_job": ["th", None], "col_job": ["th", None], "row_pass": ["lr", 2], "col_pass": ["lr", cp]}
        for e in ("fgs", "wls"):
            out.append({"name": "jobsth", "entry": e, "h": h, "w": w, "nimg": 2, "expect": expect})
    return out


MIXED = _mixed()

# single images: k_fgs_th<false, LPB> passes, 32 lines a workgroup for 4200 lines and 64 for 8300 on
# the MI355X's 256 compute units (the query asks the device); fgs entry only, the WLS filter always
# solves two right-hand sides
SINGLE = [{"name": f"th1-{o}", "entry": "fgs", "h": h, "w": w, "nimg": 1,
           "expect": {f"{a}_pass": ["th", lpb], f"{b}_pass": ["th", 16]}}
          for (h, w, o, a, b, lpb) in ((4200, 6, "rows", "row", "col", 32), (6, 4200, "cols", "col", "row", 32),
                                       (8300, 5, "rows", "row", "col", 64), (5, 8300, "cols", "col", "row", 64))]

# SDR_FGS_LR_MAXL=16 (a child process): k_fgs_lr<16>
_L16 = {"pass": ["lr", 16], "job": ["lrjob", 16]}
KNOB_MAXL16 = (_line_cases("lr16", {3: (1, 16), 100: (15, 17), 383: (1, 40), 384: (16, 17, 40)}, _L16, _L16)
               + [{"name": "lr16-map", "entry": "wls", "h": 360, "w": 560, "nimg": 2,
                   "expect": {"row_pass": ["lr", 8], "col_pass": ["lr", 16], "row_job": ["lrjob", 8],
                              "col_job": ["lrjob", 16]}}])
# SDR_FGS_LR=0 SDR_FGS_LRJOB=0 (a child process): k_fgs_th<true, LPB> passes and jobs on short lines
# ((20, 300): 16 lines a workgroup; (4200, 20): 32; (8300, 12): 64, on 256 compute units)
def _th2(n, m, lpb):
    return _line_cases(f"th2x{lpb}", {n: (m,)}, {"pass": ["th", lpb], "job": ["th", None]},
                       {"pass": ["th", 16], "job": ["th", None]})


KNOB_TH = _th2(300, 20, 16) + _th2(20, 4200, 32) + _th2(12, 8300, 64)
KNOB_ENV = {"maxl16": {"SDR_FGS_LR_MAXL": "16"}, "th": {"SDR_FGS_LR": "0", "SDR_FGS_LRJOB": "0"}}
KNOB_CASES = {"maxl16": KNOB_MAXL16, "th": KNOB_TH}

PARENT_CASES = LR4 + LR2 + TH_PAST + LR8 + STACK3 + MIXED + SINGLE
