"""sample_quantiles' Python-side validation and its binding (no GPU).

Everything the C side cannot see -- F's type, dtype and rank, q's range, out's type and shape, the
sign of the strides -- raises DomainError before a context is asked for, so it is checked here with
`context` replaced by a function that fails the test.  The header must declare
gpar_sample_quantiles, and _lib.py must bind it with the ctypes equivalents of its prototype."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

G = pytest.importorskip("gparatscale")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gpar_hip.h")).read()


@pytest.fixture
def no_library_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(G.api, "context", boom)
    monkeypatch.setattr(G.api._lib, "load", boom)


F3 = np.random.default_rng(0).standard_normal((5, 7, 3))
Q = (0.1, 0.5, 0.9)


@pytest.mark.parametrize("F", [
    F3.astype(np.float32),                 # dtype
    F3.astype(np.int64),
    F3[0, 0],                              # rank 1
    F3[None],                              # rank 4
    F3.tolist(),                           # not an array
    F3[:0],                                # no samples
    F3[:, :0],                             # no points
    F3[::-1],                              # a negative stride
    np.broadcast_to(F3[:1], (4, 7, 3)),    # a zero stride
], ids=["float32", "int64", "rank1", "rank4", "list", "S=0", "n=0", "negative", "broadcast"])
def test_bad_samples_raise_before_the_library(no_library_call, F):
    with pytest.raises(G.DomainError):
        G.sample_quantiles(F, Q)


@pytest.mark.parametrize("q", [(-0.1,), (1.1,), (float("nan"),), (0.5, 2.0), (), ("a",),
                               (0.5, float("inf"))],
                         ids=["-0.1", "1.1", "nan", "one bad", "empty", "text", "inf"])
def test_bad_levels_raise_before_the_library(no_library_call, q):
    with pytest.raises(G.DomainError):
        G.sample_quantiles(F3, q)
    with pytest.raises(G.DomainError):
        G.sample_quantiles(F3[:, :, 0], q)


@pytest.mark.parametrize("out", [
    np.zeros((2, 7, 3)),                   # nq
    np.zeros((3, 7)),                      # rank
    np.zeros((3, 3, 7)),                   # transposed shape
    np.zeros((3, 7, 3), dtype=np.float32),
    [[0.0] * 3] * 7,
    np.zeros((3, 7, 3))[:, ::-1],          # a negative stride
], ids=["nq", "rank", "shape", "float32", "list", "negative"])
def test_bad_out_raises_before_the_library(no_library_call, out):
    with pytest.raises(G.DomainError):
        G.sample_quantiles(F3, Q, out=out)


def test_read_only_out_raises_before_the_library(no_library_call):
    out = np.zeros((3, 7, 3))
    out.setflags(write=False)
    with pytest.raises(G.DomainError):
        G.sample_quantiles(F3, Q, out=out)


def test_domain_error_is_a_value_error(no_library_call):
    with pytest.raises(ValueError):
        G.sample_quantiles(F3, (1.5,))


def test_signatures():
    p = inspect.signature(G.sample_quantiles).parameters
    assert list(p) == ["F", "q", "out", "device"]
    assert (p["out"].default, p["device"].default) == (None, 0)
    p = inspect.signature(G.Posterior.sample_chain_quantiles).parameters
    assert list(p) == ["self", "t_star", "given_inputs", "samples", "quantiles", "seed"]
    assert p["seed"].default == 0


C_TO_CTYPES = {"gpar_ctx*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64,
               "const double*": C.c_void_p, "double*": C.c_void_p}


def test_header_declares_and_lib_binds_the_entry_point():
    src = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"int32_t\s+gpar_sample_quantiles\s*\(([^;]*?)\)\s*;", src, re.S)
    assert m, "include/gpar_hip.h does not declare gpar_sample_quantiles"
    params = []
    for a in m.group(1).split(","):
        typ, name = re.match(r"(.*?)\s*(\w+)$", " ".join(a.split())).groups()
        params.append((typ.replace(" *", "*"), name))
    assert [n for _, n in params] == ["ctx", "samples", "n", "p", "f", "ld_s", "ld_r", "ld_c", "nq",
                                      "q", "mem", "out", "ldo_q", "ldo_r", "ldo_c"]
    assert [t for t, _ in params] == ["gpar_ctx*", "int32_t", "int64_t", "int64_t", "const double*",
                                      "int64_t", "int64_t", "int64_t", "int32_t", "const double*",
                                      "int32_t", "double*", "int64_t", "int64_t", "int64_t"]
    assert re.search(r"#define GPAR_ABI_VERSION 1\b", HEADER)   # the change only adds
    assert "gpar_sample_quantiles" in G.EXPORTED
    f = G.load().gpar_sample_quantiles
    assert f.restype is C.c_int32
    assert list(f.argtypes) == [C_TO_CTYPES[t] for t, _ in params]


def test_counters_are_known_names():
    assert G.debug_counter("quantile_reg") >= 0 and G.debug_counter("quantile_lds") >= 0
    assert G.debug_counter("quantile_nope") == -1
