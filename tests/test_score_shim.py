"""The scorers' Julia bindings, checked without a GPU: the shim exports sample_scores and
gaussian_scores, each body makes one ccall of its entry point, and the ccall's argument types are
the Julia equivalents of the header's prototype, one for one."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "julia", "GPARatScaleHIP.jl")
HEADER = os.path.join(ROOT, "include", "gpar_hip.h")

C_TO_JL = {"gpar_ctx*": "Ptr{Cvoid}", "int32_t": "Int32", "int64_t": "Int64",
           "const double*": "Ptr{Float64}", "double*": "Ptr{Float64}", "int32_t*": "Ptr{Int32}",
           "int64_t*": "Ptr{Int64}"}


def _shim():
    return re.sub(r"#=.*?=#", "", open(SHIM).read(), flags=re.S)


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, f"include/gpar_hip.h does not declare {name}"
    out = []
    for a in m.group(1).split(","):
        typ, _ = re.match(r"(.*?)\s*(\w+)$", " ".join(a.split())).groups()
        out.append(typ.replace(" *", "*"))
    return out


def _split_top(s):
    out, depth, cur = [], 0, []
    for ch in s:
        depth += ch in "([{"
        depth -= ch in ")]}"
        if ch == "," and depth == 0:
            out.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    out.append("".join(cur).strip())
    return [x for x in out if x]


def _ccall(body):
    i = body.index("ccall(") + len("ccall")
    depth = 0
    for j in range(i, len(body)):
        depth += body[j] == "("
        depth -= body[j] == ")"
        if depth == 0:
            return _split_top(body[i + 1:j])
    raise AssertionError("unbalanced ccall")


def test_shim_exports_the_scorers():
    exported = re.search(r"^export ([\w,\s]+?)\n\n", _shim(), re.M).group(1)
    names = [s.strip() for s in exported.split(",")]
    assert "sample_scores" in names and "gaussian_scores" in names
    assert "sample_quantiles" in names and "select_pseudo_inputs" in names   # nothing dropped


@pytest.mark.parametrize("fn,sym,positional", [
    ("sample_scores", "gpar_score_samples", ["F", "y"]),
    ("gaussian_scores", "gpar_score_gaussian", ["mean", "std", "y"]),
])
def test_scorer_calls_its_entry_point_with_the_headers_types(fn, sym, positional):
    m = re.search(r"^function %s\((.*?)\)\n(.*?)\nend\n" % fn, _shim(), re.M | re.S)
    assert m, f"{fn} is not defined"
    sig, body = m.group(1), m.group(2)
    pos, _, kw = sig.partition(";")
    assert [a.split("::")[0].strip() for a in _split_top(pos)] == positional
    assert re.search(r"levels\s*=\s*\(0\.5, 0\.9, 0\.95\)", kw)
    assert re.search(r"bins::Integer\s*=\s*10", kw)
    assert body.count("ccall(") == 1
    parts = _ccall(body)
    assert parts[0] == f"(:{sym}, libgpar)" and parts[1] == "Int32"
    types = _split_top(parts[2][1:-1])
    assert types == [C_TO_JL[t] for t in _prototype(sym)]
    assert len(parts[3:]) == len(types)
    assert "GPAR_MEM_HOST" in body
