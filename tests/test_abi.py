"""CPU: the C-ABI library builds, loads, and exports every symbol include/eps_abi.h declares
(no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "eps_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(eps_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_expected_surface():
    syms = declared_symbols()
    for s in ["eps_pair_scores", "eps_pair_scores_f64", "eps_spmm_csr", "eps_mlp_decode", "eps_gemm_f32",
              "eps_col_sums", "eps_node_weights", "eps_gcn_norm", "eps_pack_keys", "eps_unpack_keys",
              "eps_last_error", "eps_version"]:
        assert s in syms


def test_library_exports_every_declared_symbol(eps):
    lib = eps.load()
    for s in declared_symbols():
        assert hasattr(lib, s), f"{s} declared in eps_abi.h but not exported"
    assert lib.eps_version() == eps._lib.ABI_VERSION == 7


def _kind(c_type):
    """The ctypes-level kind of a C type of the header: every pointer is one kind; int32_t and int are one ctypes type here."""
    c_type = re.sub(r"\bconst\b", "", c_type).strip()
    if "*" in c_type or "[" in c_type:
        return "pointer"
    return {"int": "int32", "int32_t": "int32", "int64_t": "int64", "uint32_t": "uint32", "float": "float", "double": "double"}[c_type]


def _ctypes_kind(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int32: "int32", ctypes.c_int: "int32", ctypes.c_int64: "int64", ctypes.c_uint32: "uint32",
            ctypes.c_float: "float", ctypes.c_double: "double"}[t]


def declared_prototypes():
    """name -> (return kind, [argument kinds]) of every ``ret name(args);`` of the header, comments stripped."""
    text = open(os.path.join(ROOT, "include", "eps_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    protos = {}
    for ret, name, args in re.findall(r"^[ \t]*((?:const[ \t]+)?\w+[ \t\*]+)(eps_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        args = [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
        # an argument is "type name": drop the trailing identifier, keep any * that sticks to it
        kinds = [_kind(re.sub(r"\b[A-Za-z_]\w*\s*(\[\s*\])?$", lambda m: m.group(1) or "", a)) for a in args]
        assert name not in protos, f"{name} declared twice"
        protos[name] = (_kind(ret), kinds)
    return protos


def test_python_signatures_cover_header(eps):
    """_lib.SIGNATURES mirrors the header by hand: same names, and per symbol the same return kind, the same number of arguments
    and the same kind per argument (a wrong width or a missing argument there corrupts a call silently)."""
    assert sorted(eps._lib.SIGNATURES) == declared_symbols()
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols(), "a declaration of eps_abi.h was not parsed as a prototype"
    for name, (ret, kinds) in sorted(protos.items()):
        res, args = eps._lib.SIGNATURES[name]
        assert _ctypes_kind(res) == ret, f"{name}: returns {ret} in the header, {res.__name__} in SIGNATURES"
        assert len(args) == len(kinds), f"{name}: {len(kinds)} arguments in the header, {len(args)} in SIGNATURES"
        for i, (a, kd) in enumerate(zip(args, kinds)):
            assert _ctypes_kind(a) == kd, f"{name}: argument {i} is {kd} in the header, {a.__name__} in SIGNATURES"


def test_every_unit_of_the_library_is_warmed():
    """eps_abi.h promises that eps_warm_up loads EVERY code object: each source the Makefile compiles, other than eps_common.hip
    itself, defines eps_warm_<stem>, and the one list eps_warm_up declares and calls from (EPS_UNITS) names exactly those stems.
    Text only: a unit added to SRCS and forgotten there pays its code-object load inside its first timed call."""
    csrc = os.path.join(ROOT, "edge-proposal-sets_amd", "csrc")
    srcs = re.search(r"^SRCS\s*:?=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    stems = [s[:-len(".hip")] for s in srcs if s != "eps_common.hip"]
    assert len(stems) == len(srcs) - 1 and len(set(stems)) == len(stems)
    for stem in stems:
        text = open(os.path.join(csrc, stem + ".hip")).read()
        assert re.search(r'^extern "C" void eps_warm_%s\(void \*stream\)\s*\{' % stem, text, flags=re.M), f"{stem}.hip defines no eps_warm_{stem}"
        assert re.search(r"^__global__ void %s_warm_kernel\(\) \{\}" % stem, text, flags=re.M), f"{stem}.hip has no kernel to launch"
    common = open(os.path.join(csrc, "eps_common.hip")).read()
    units = re.search(r"^#define EPS_UNITS\(X\)((?:.*\\\n)*.*)$", common, flags=re.M).group(1)
    listed = re.findall(r"\bX\((\w+)\)", units)
    assert sorted(listed) == sorted(stems) and len(set(listed)) == len(listed)
    assert "eps_warm_" not in re.sub(r"eps_warm_##unit|eps_warm_up|eps_warm_<unit>", "", common), "a warm call outside the list"


def test_argument_validation_without_gpu(eps):
    """EINVAL paths return before any HIP call, so they are checkable on a CPU-only box."""
    lib = eps.load()
    rc = lib.eps_pair_scores(None, None, None, None, 10, None, None, 5, None, None, None, None)
    assert rc == -1 and b"null" in lib.eps_last_error()
    rc = lib.eps_mlp_decode(None, 0, 102, None, None, 0, None, None, 2, 1, None, None)
    assert rc == -1 and b"hdim" in lib.eps_last_error()
    rc = lib.eps_spmm_csr(None, None, None, -1, None, 0, 0, None, 0, 0, None, 0, None)
    assert rc == -1


def test_ops_refuse_cpu_tensors(eps):
    import torch
    g = eps.add_edges("ddi", torch.tensor([[0, 1], [1, 2]]), torch.ones(2), torch.zeros(2, 0, dtype=torch.long), 3)
    with pytest.raises(eps.EpsError):
        eps.ops.pair_scores(g.rowptr, g.col, None, None, 3, torch.zeros(1, dtype=torch.int32),
                            torch.zeros(1, dtype=torch.int32))
    if not torch.cuda.is_available():
        with pytest.raises(eps.EpsError):
            eps.AA(g, torch.tensor([[0], [2]]))


def test_missing_library_fails_loudly(eps, monkeypatch, tmp_path):
    """No HIP library -> the loader raises (there is no CPU fallback to slide onto)."""
    from eps_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libeps_hip.so"))
    with pytest.raises(_lib.EpsError, match="no CPU fallback"):
        _lib.load()


def test_product_package_never_imports_the_oracle():
    import glob
    for f in glob.glob(os.path.join(ROOT, "edge-proposal-sets_amd", "*.py")) + [os.path.join(ROOT, n) for n in ("filter.py", "rank.py", "eps_amd.py")]:
        src = open(f).read()
        assert "import oracle" not in src and "from oracle" not in src and "eps_oracle" not in src, f


def test_graft_entry_build():
    """The driver's "does it build" check: __graft_entry__.build() compiles the library, the oracle and the example host and
    verifies the ABI version the Python side expects (an incremental make here)."""
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    entry = importlib.import_module("__graft_entry__")
    entry.build()
