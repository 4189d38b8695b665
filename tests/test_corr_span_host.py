"""Host arithmetic of the "corr_span" plan (csrc/span.hpp through gpar_corr_span_plan /
gpar_corr_span_psi; no device work): span counts, the default rule and the chunk transitions
composed over spans, against numpy."""
import ctypes as C

import numpy as np
import pytest

G = pytest.importorskip("gparatscale")
from gparatscale import _lib as L  # noqa: E402


def plan(knob, split, n, mp, outputs=63):
    span, nsp = C.c_int32(), C.c_int64()
    code = L.load().gpar_corr_span_plan(knob, split, outputs, n, mp, C.byref(span), C.byref(nsp))
    return code, span.value, nsp.value


@pytest.mark.parametrize("s", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 300, 3 * 4 * 256 + 37, 1024, 1025, 1_000_000])
def test_span_counts(s, n):
    code, span, nsp = plan(s, 1, n, 128)
    assert code == L.GPAR_OK and span == s
    nch = -(-n // 256)
    assert nsp == -(-nch // s) == -(-n // (256 * s))   # what the Gram derives from L = 256 S


def test_default_rule_and_bad_values():
    # auto: only fit calls of more than 16 outputs (the round-by-round split fit) that take the CU
    # split by its size gate (N Mp^2 >= 1e11) leave 1
    _, auto_big, _ = plan(-1, 1, 1_000_000, 512)
    assert auto_big in (1, 2, 4, 8)
    assert plan(-1, 1, 1_000_000, 512, outputs=17)[1] == auto_big
    assert plan(-1, 1, 1_000_000, 512, outputs=16)[1] == 1     # the round overlap's range
    assert plan(-1, 1, 1_000_000, 512, outputs=8)[1] == 1
    assert plan(2, 1, 1_000_000, 512, outputs=8)[1] == 2       # a set value holds there too
    assert plan(-1, 0, 1_000_000, 512)[1] == 1      # unsplit
    assert plan(-1, 1, 100_000, 512)[1] == 1        # forced split below the gate (2.6e10)
    assert plan(-1, 1, 805, 128)[1] == 1
    assert plan(4, 0, 805, 128)[1] == 4             # a set value holds anywhere
    for bad in (0, 3, 5, 16, -2):
        assert plan(bad, 1, 1000, 128)[0] == L.GPAR_ERR_ARG


@pytest.mark.parametrize("sdim", [1, 2, 3])
@pytest.mark.parametrize("s", [1, 2, 4, 8])
@pytest.mark.parametrize("nch", [1, 4, 13])
def test_psi_composition(sdim, s, nch):
    rng = np.random.default_rng(100 * sdim + 10 * s + nch)
    phi = rng.uniform(-0.9, 0.9, size=(nch, sdim, sdim))
    nsp = -(-nch // s)
    pre = np.full((nch, sdim, sdim), np.nan)
    tot = np.full((nsp, sdim, sdim), np.nan)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.load().gpar_corr_span_psi(sdim, nch, s, vp(phi), vp(pre), vp(tot)) == L.GPAR_OK
    # the chunk carry cin[j + 1] = Phi_j cin[j] + send[j] restricted to one span
    for J in range(nsp):
        p = np.eye(sdim)
        for j in range(J * s, min(nch, J * s + s)):
            np.testing.assert_allclose(pre[j], p, rtol=1e-14, atol=1e-16)
            p = phi[j] @ p
        np.testing.assert_allclose(tot[J], p, rtol=1e-14, atol=1e-16)
    # carrying a state over the spans equals carrying it over the chunks
    c = rng.normal(size=sdim)
    by_chunk = c.copy()
    for j in range(nch):
        by_chunk = phi[j] @ by_chunk
    by_span = c.copy()
    for J in range(nsp):
        by_span = tot[J] @ by_span
    np.testing.assert_allclose(by_span, by_chunk, rtol=1e-12, atol=1e-15)
