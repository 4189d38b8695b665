"""The pseudo-input selector's bindings, checked without a GPU: the Julia shim exports
select_pseudo_inputs and its body ccalls gpar_select_pseudo_inputs (tests/test_julia_shim.py then
type-checks that call against the header's prototype), the header, the ctypes table and the Python
API name it, and the reference's five signatures are untouched."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "julia", "GPARatScaleHIP.jl")
HEADER = os.path.join(ROOT, "include", "gpar_hip.h")


def _shim():
    return re.sub(r"#=.*?=#", "", open(SHIM).read(), flags=re.S)


def test_shim_exports_select_pseudo_inputs_and_calls_the_library():
    src = _shim()
    exported = re.search(r"^export ([\w,\s]+?)\n\n", src, re.M).group(1)
    assert "select_pseudo_inputs" in [s.strip() for s in exported.split(",")]
    m = re.search(r"^function select_pseudo_inputs\((.*?)\)\n(.*?)\nend\n", src, re.M | re.S)
    assert m, "select_pseudo_inputs is not defined"
    sig, body = m.group(1), m.group(2)
    pos, _, kw = sig.partition(";")
    assert [a.strip() for a in pos.split(",")] == ["input_locations", "pseudo_input_locations"]
    assert re.search(r"iters::Integer\s*=\s*10", kw) and re.search(r"snap::Bool\s*=\s*true", kw)
    assert body.count("ccall(") == 1
    assert "ccall((:gpar_select_pseudo_inputs, libgpar), Int32," in body
    assert "GPAR_MEM_HOST" in body


def test_header_and_python_name_the_entry_point():
    import gparatscale as G
    header = open(HEADER).read()
    assert re.search(r"int32_t gpar_select_pseudo_inputs\(gpar_ctx\* ctx, int64_t n, int64_t d,",
                     header)
    assert "#define GPAR_ABI_VERSION 1" in header          # the change only adds
    assert "gpar_select_pseudo_inputs" in G.EXPORTED
    assert callable(G.select_pseudo_inputs)
    import inspect
    params = inspect.signature(G.select_pseudo_inputs).parameters
    assert list(params) == ["V", "Z0_or_M", "iters", "snap", "seed", "device"]
    assert (params["iters"].default, params["snap"].default, params["seed"].default,
            params["device"].default) == (10, True, 0, 0)
