"""The filter's refusals that need no device (csrc/sdr_wls_plan.hip's one rule) through the entries
that apply it: sdr_wls_create, sdr_fgs_filter_device and sdr_fgs_plan_query.  The status codes, and
that one condition reads the same through every entry.  The pointers are dummies: every case
returns before the first HIP call."""
import ctypes

import pytest

from stereo_depth_ruler_amd import _lib
from stereo_depth_ruler_amd._lib import FGS_PCR, FGS_THOMAS

ARG, SIZE = -1, -4
DUMMY = ctypes.c_void_p(0x1000)
CUS = 256


def last_error():
    return _lib.lib().sdr_last_error().decode()


def wls_params(**kw):
    """createDisparityWLSFilter's defaults for minDisparity 0, 64 disparities, blockSize 5."""
    p = _lib.WlsParams(8000.0, 1.5, 24, 3, 0.001, 0.25, 3, 64, 0, 0, 0, 0, FGS_THOMAS)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def create(**kw):
    """(status, text) of sdr_wls_create; a handle must not come back."""
    h = ctypes.c_void_p()
    rc = _lib.lib().sdr_wls_create(ctypes.byref(wls_params(**kw)), 0, ctypes.byref(h))
    assert rc != 0 and not h.value
    return rc, last_error()


def fgs(w=40, h=30, lambda_=8000.0, sigma=1.5, att=0.25, iters=3, solver=FGS_THOMAS, nimg=2):
    rc = _lib.lib().sdr_fgs_filter_device(DUMMY, w, w, h, lambda_, sigma, att, iters, DUMMY, nimg, solver, None)
    return rc, last_error()


def query(w, h, solver, num_iter=3):
    p = _lib.FgsPlan()
    rc = _lib.lib().sdr_fgs_plan_query(w, h, 1, 2, num_iter, solver, CUS, ctypes.byref(p))
    return rc, (last_error() if rc else ""), p


# (the condition, sdr_wls_params fields, sdr_fgs_filter_device arguments)
PARAMS = [
    ("lambda < 0", dict(lambda_=-1.0), dict(lambda_=-1.0)),
    ("lambda NaN", dict(lambda_=float("nan")), dict(lambda_=float("nan"))),
    ("sigma < 0", dict(sigma_color=-0.5), dict(sigma=-0.5)),
    ("num_iter 0", dict(num_iter=0), dict(iters=0)),
    ("solver 7", dict(fgs_solver=7), dict(solver=7)),
    # 8000 * 4^k passes 2^100 at k = 44
    ("Thomas, attenuation 4", dict(lambda_attenuation=4.0, num_iter=50), dict(att=4.0, iters=50)),
    ("Thomas, attenuation < 0", dict(lambda_attenuation=-0.25, num_iter=2), dict(att=-0.25, iters=2)),
]


@pytest.mark.parametrize("what,wls,scalars", PARAMS, ids=[c[0] for c in PARAMS])
def test_parameter_refusals(what, wls, scalars):
    rc_c, text_c = create(**wls)
    rc_f, text_f = fgs(**scalars)
    print(what, rc_c, repr(text_c), rc_f, repr(text_f))
    assert (rc_c, rc_f) == (ARG, ARG)
    assert text_c == text_f


def test_thomas_range_counts_every_iteration():
    """8000 * 4^44 is the first lambda past 2^100: 45 iterations reach it."""
    assert create(lambda_attenuation=4.0, num_iter=45)[0] == ARG
    assert fgs(att=4.0, iters=45)[0] == ARG


def test_solver_text_is_one():
    _, text_c = create(fgs_solver=7)
    _, text_f = fgs(solver=7)
    rc_q, text_q, _ = query(5, 5, 7)
    print(repr(text_c), repr(text_f), repr(text_q))
    assert rc_q == ARG
    assert text_c == text_f == text_q


@pytest.mark.parametrize("field", ["depth_discontinuity_radius", "left_offset", "right_offset", "top_offset",
                                   "bottom_offset"])
def test_negative_radius_or_offset(field):
    rc, text = create(**{field: -1})
    print(field, rc, repr(text))
    assert rc == ARG
    assert text == create(depth_discontinuity_radius=-2)[1]


def test_refusals_keep_their_order():
    """lambda, sigma and num_iter win over the solver, the solver over a negative radius."""
    assert create(lambda_=-1.0, fgs_solver=7)[1] == create(lambda_=-1.0)[1]
    assert create(fgs_solver=7, left_offset=-1)[1] == create(fgs_solver=7)[1]
    assert fgs(w=4097, h=3, solver=FGS_PCR, iters=0)[0] == ARG


def test_pcr_line_limit():
    rc, _, p = query(4096, 3, FGS_PCR)
    assert rc == 0 and p.row_pass.as_tuple() == ("pcr", 1) and p.col_pass.as_tuple()[0] == "pcr"
    texts = []
    for w, h in ((4097, 3), (3, 4097)):
        rc_f, text_f = fgs(w=w, h=h, solver=FGS_PCR)
        rc_q, text_q, _ = query(w, h, FGS_PCR)
        print(w, h, rc_f, repr(text_f), rc_q, repr(text_q))
        assert (rc_f, rc_q) == (SIZE, SIZE)
        texts += [text_f, text_q]
    # the sequential solver takes the shape
    assert query(4097, 3, FGS_THOMAS)[0] == 0
    assert len(set(texts)) == 1
