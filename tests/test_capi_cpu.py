"""CPU-side checks of the drop-in boundary: the shared library builds, loads and exports every
symbol include/bsed.h declares, and the binding _lib.py derives from the header agrees with it (argument and return
types, struct layouts and constants as the C compiler sees them).  No compute call is made here (no GPU in this tier)."""
import ctypes
import keyword
import os
import re
import shutil
import subprocess

import pytest

import bsed_amd
from bsed_amd import _lib as L


def test_library_is_built_in_tree():
    assert os.path.exists(L.LIB_PATH), "run __graft_entry__.build() first"
    assert os.path.dirname(L.LIB_PATH).endswith("bird-sound-event-detecion_amd")


def test_every_header_symbol_is_exported():
    names = L.header_symbols()
    assert "bsed_mel_linear" in names and "bsed_last_error" in names
    lib = ctypes.CDLL(L.LIB_PATH)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in include/bsed.h but not exported: {missing}"


def test_error_convention_without_gpu():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 1
    assert b"gfx950" in lib.bsed_build_info()
    # argument validation happens before any HIP call: NULL plan -> negative code + message
    rc = lib.bsed_mel_linear(None, None, 1, 32000, None, None, None, None, None)
    assert rc < 0 and b"null" in lib.bsed_last_error()


def test_step_state_pointers_are_set_or_cleared_together():
    """bsed_set_step_state (ABI 3: seed addend, step addend, learning rate) only stores pointers -- no HIP call -- and
    refuses a mix of null and non-null ones: a half-armed library would replay a graph with one scalar still baked"""
    lib = L.lib()
    assert lib.bsed_abi_version() >= 3
    assert len(L.FUNCTIONS["bsed_set_step_state"][1]) == 3
    assert lib.bsed_set_step_state(None, None, None) == 0
    for mixed in ((64, None, None), (None, 64, 64), (64, 64, None)):
        assert lib.bsed_set_step_state(*mixed) < 0 and b"together" in lib.bsed_last_error()
    assert lib.bsed_set_step_state(None, None, None) == 0


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bsed_amd.features import MelFrontEnd
    with pytest.raises(L.BsedError):
        MelFrontEnd()


def _prototypes():
    """(name, return type text, [parameter texts]) of every prototype in include/bsed.h, by a scan of its own"""
    txt = re.sub(r"/\*.*?\*/", " ", open(L.HEADER_PATH).read(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r"([\w *]+?)\s*\b(bsed_\w+)\s*\(([^()]*)\)\s*;", txt):
        params = " ".join(params.split())
        out.append((name, re.sub(r"\s*\*", "*", " ".join(ret.split())), [] if params == "void" else params.split(",")))
    return out


def test_every_prototype_is_bound_from_the_header():
    scalars = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
               "float": ctypes.c_float, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32,
               "uint64_t": ctypes.c_uint64}
    protos = _prototypes()
    assert sorted(n for n, _, _ in protos) == L.header_symbols() and len(protos) > 90
    lib = L.lib()
    for name, ret, params in protos:
        fn = getattr(lib, name)
        want_ret = None if ret == "void" else ctypes.c_char_p if ret == "const char*" else scalars[ret]
        assert fn.restype is want_ret, (name, ret, fn.restype)
        want = [ctypes.c_void_p if "*" in p else scalars[" ".join(p.split()[:-1])] for p in params]
        assert fn.argtypes == want, (name, params, fn.argtypes)


@pytest.mark.skipif(not (shutil.which("cc") or shutil.which("gcc")), reason="no host C compiler")
def test_struct_layouts_and_constants_match_the_c_compiler(tmp_path):
    assert set(L.STRUCTS) == {"BsedMelCfg", "BsedIgemmDesc", "BsedPackJob", "BsedWgradDesc", "BsedReduceJob",
                              "BsedBnEvalJob", "BsedHeadBwdDesc", "BsedGluDesc", "BsedGluPlan", "BsedContractPlan"}
    assert {"BSED_EPI_PLAIN", "BSED_EPI_STATS", "BSED_EPI_GLU_POOL", "BSED_EPI_GLU_BWD", "BSED_EPI_ADD_STATS2",
            "BSED_PACK_MAX_JOBS", "BSED_REDUCE_MAX_JOBS", "BSED_BN_EVAL_MAX_JOBS"} <= set(L.CONSTANTS)
    lines, want = [], []
    for sname, S in L.STRUCTS.items():
        lines.append(f'printf("S {sname} %zu\\n", sizeof({sname}));')
        want.append(f"S {sname} {ctypes.sizeof(S)}")
        for fname, _ in S._fields_:
            c = fname[:-1] if fname.endswith("_") and keyword.iskeyword(fname[:-1]) else fname
            lines.append(f'printf("F {sname}.{fname} %zu %zu\\n", offsetof({sname}, {c}), sizeof((({sname}*)0)->{c}));')
            f = getattr(S, fname)
            want.append(f"F {sname}.{fname} {f.offset} {f.size}")
    for k, v in L.CONSTANTS.items():
        lines.append(f'printf("K {k} %lld\\n", (long long)({k}));')
        want.append(f"K {k} {v}")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bsed.h"\nint main(void) {\n  '
                   + "\n  ".join(lines) + "\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    cc = shutil.which("cc") or shutil.which("gcc")
    subprocess.run([cc, "-std=c11", "-I", os.path.dirname(L.HEADER_PATH), str(src), "-o", exe], check=True, timeout=120)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert got == want


def test_wrong_argument_type_fails_before_the_library():
    with pytest.raises(ctypes.ArgumentError):
        L.lib().bsed_mel_linear(None, None, 1.5, 32000, None, None, None, None, None)   # float for `int B`


def test_header_parser_refuses_what_it_does_not_know(tmp_path):
    for decl in ("int bsed_f(short n);", "typedef struct BsedX { unsigned n; } BsedX;", "int (*bsed_g)(int);",
                 "#define BSED_NAME \"text\""):
        h = tmp_path / "h.h"
        h.write_text(decl + "\n")
        with pytest.raises(L.BsedError):
            L.parse_header(str(h))


# ---- tile-geometry validation of the contraction entry points: every check runs before the first HIP call ----
_CONV_ENTRIES = ("bsed_igemm", "bsed_igemm3", "bsed_igemm3s", "bsed_igemm3n", "bsed_wgrad", "bsed_wgrad3")
_GEOMETRY_DEFECTS = {
    "TW=3": dict(TW=3),
    "TW does not divide W": dict(W=24),
    "TH*TW != 128": dict(TH=4),
    "tap outside the halo": dict(dh0=-2),
    "ntaps=10": dict(ntaps=10),
    "NP not a multiple of 32": dict(NP=48),
}


def _conv_desc(entry, TW=16, TH=8, W=16, dh0=-1, ntaps=9, NP=32):
    """A 3 x 3, 32 -> 32 channel contraction over (2, 16, 16) that every entry point accepts, with dummy non-null
    pointers (never dereferenced on the host), except for what the keyword arguments break."""
    wg = entry.startswith("bsed_wgrad")
    d = L.STRUCTS["BsedWgradDesc" if wg else "BsedIgemmDesc"]()
    dummy = 0x1000
    d.in_ = dummy
    d.in_pitch = 32
    d.NB, d.H, d.W, d.CIN, d.N, d.NP = 2, 16, W, 32, 32, NP
    d.TH, d.TW, d.hh, d.hw = TH, TW, 1, 1
    d.ntaps = ntaps
    for i in range(9):
        d.dh[i], d.dw[i] = i // 3 - 1, i % 3 - 1
    d.dh[0] = dh0
    if wg:
        d.dy = d.part = dummy
        d.dy_pitch, d.CINP, d.G = 32, 32, 1
    else:
        d.w = d.out = dummy
        d.out_pitch = d.e_pitch = 32
        d.ph = d.pw = 1
        d.Hp, d.Wp = 16, W
        d.epilogue = L.CONSTANTS["BSED_EPI_PLAIN"]
    return d


@pytest.mark.parametrize("defect", list(_GEOMETRY_DEFECTS))
@pytest.mark.parametrize("entry", _CONV_ENTRIES)
def test_ill_formed_tile_geometry_is_rejected_before_any_hip_call(entry, defect):
    lib = L.lib()
    d = _conv_desc(entry, **_GEOMETRY_DEFECTS[defect])
    d.G = 1                                                       # bsed_igemm3s reads its grid size from the descriptor
    rc = getattr(lib, entry)(ctypes.byref(d), None)
    msg = lib.bsed_last_error().decode()
    assert rc == -1, (entry, defect, rc, msg)                     # BSED_ERR_ARG: no HIP call was reached
    # wgrad_prepare serves both weight-gradient entries and reports as bsed_wgrad
    prefix = "bsed_wgrad:" if entry == "bsed_wgrad3" else entry + ":"
    assert msg.startswith(prefix), (entry, defect, msg)
