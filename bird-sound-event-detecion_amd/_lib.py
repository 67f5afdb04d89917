"""ctypes binding of libbsed.so (C ABI declared in include/bsed.h).

The library is built in-tree by ``csrc/build.sh`` (``__graft_entry__.build()``) and is the ONLY
compute path: ``lib()`` raises if it is missing -- there is no eager/PyTorch fallback.
"""
import ctypes
import keyword
import os
import re

# The train step keeps up to four HIP streams busy (main, GRU weight gradients, the next batch's mel transform, the EMA
# teacher) and RCCL adds its own.  The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4):
# beyond that two streams share a queue and their kernels serialise, which takes the overlap back -- measured on one
# MI355X box, same process otherwise: 13.28 ms per step; 13.63 once an RCCL communicator exists; 13.31 with 8 queues
# (DESIGN.md section 7).  Read by the runtime when it initialises, so it is set at import, before the first HIP call;
# an explicit setting in the environment wins; importing after the runtime is up only warns (import order is not an API:
# launch scripts and the profiling tools under tools/ export the variable themselves).
def _hw_queue_default():
    if "GPU_MAX_HW_QUEUES" in os.environ:
        return
    import sys
    t = sys.modules.get("torch")
    if t is not None and getattr(t, "cuda", None) is not None and t.cuda.is_initialized():
        # too late: the runtime has read its configuration.  Say so instead of silently running on 4 queues.
        import warnings
        warnings.warn("bsed_amd was imported after the HIP runtime was initialised and GPU_MAX_HW_QUEUES is not set: the "
                      "train step's streams and RCCL's will share the default 4 hardware queues (2.5-3.4 % slower steps "
                      "once an RCCL communicator exists, DESIGN.md section 7).  Export GPU_MAX_HW_QUEUES=8 in the "
                      "launch environment, or import bsed_amd before the first torch.cuda call.", RuntimeWarning)
        return
    os.environ["GPU_MAX_HW_QUEUES"] = "8"


_hw_queue_default()

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BSED_LIB_PATH") or os.path.join(_HERE, "libbsed.so")  # override: A/B experiment builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bsed.h")

_lib = None


class BsedError(RuntimeError):
    pass


# include/bsed.h is the one statement of the C ABI: the prototypes (-> argtypes / restype), the descriptor structs (->
# ctypes.Structure classes) and the integer constants are read from it, never restated in Python, so a change there
# reaches every caller or fails loudly.  The grammar is the header's own -- prototypes, `typedef struct X {...} X;`,
# enums and `#define NAME <int>` -- over the scalar types below and pointers (void*); anything else raises with the
# offending text.
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double, "char": ctypes.c_char,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
_ITEM = re.compile(r"""(?: typedef\s+struct\s+\w+\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)\s*;
                        | enum\s*\{(?P<enum>[^{}]*)\}\s*;
                        | (?P<ret>[\w\s*]+?)\s*\b(?P<fn>\w+)\s*\((?P<params>[^()]*)\)\s*; )\s*""", re.X)


def _unparsed(text):
    return BsedError(f"include/bsed.h: cannot bind {' '.join(text.split())!r}")


def _ctype(base, stars, text):
    if stars:
        return ctypes.c_void_p
    base = " ".join(w for w in base.split() if w != "const")
    if base not in _SCALARS:
        raise _unparsed(text)
    return _SCALARS[base]


def _declaration(text):
    """'const float *a, *b' / 'int dh[9]' -> [(name, ctype, array length or 0), ...]"""
    head, *more = text.split(",")
    m = re.fullmatch(r"\s*([\w\s]+?)(\s*\**\s*\w+\s*(?:\[\d+\])?\s*)", head)
    out = []
    for d in [m and m[2]] + more:
        dm = d and re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
        if not dm:
            raise _unparsed(text)
        out.append((dm[2], _ctype(m[1], dm[1], text), int(dm[3] or 0)))
    return out


def _param(text):
    (_, t, n), = _declaration(text)
    if n:
        raise _unparsed(text)
    return t


def parse_header(path=None):
    """include/bsed.h -> (functions {name: (restype, [argtypes])}, structs {name: Structure}, constants {name: int})"""
    txt = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(path or HEADER_PATH).read(), flags=re.S)
    txt = re.sub(r"#ifdef __cplusplus.*?#endif", " ", txt, flags=re.S)     # the extern "C" guard
    functions, structs, constants = {}, {}, {}
    for line in re.findall(r"^[ \t]*#.*", txt, flags=re.M):
        d = re.fullmatch(r"\s*#\s*define\s+(\w+)(?:\s+(-?\d+))?\s*", line)
        if d and d[2]:
            constants[d[1]] = int(d[2])
        elif not (d or re.fullmatch(r"\s*#\s*(ifndef|endif|include)\b.*", line)):
            raise _unparsed(line)
    txt = re.sub(r"^[ \t]*#.*", " ", txt, flags=re.M).strip()
    pos = 0
    while pos < len(txt):
        m = _ITEM.match(txt, pos)
        if not m:
            raise _unparsed(txt[pos:pos + 120])
        pos = m.end()
        if m["struct"]:
            fields = [f for decl in m["fields"].split(";") if decl.strip() for f in _declaration(decl)]
            structs[m["struct"]] = type(m["struct"], (ctypes.Structure,), {"_fields_": [
                (n + "_" if keyword.iskeyword(n) else n, t * k if k else t) for n, t, k in fields]})
        elif m["enum"] is not None:
            v = -1
            for e in filter(str.strip, m["enum"].split(",")):
                em = re.fullmatch(r"\s*(\w+)\s*(?:=\s*(-?\d+)\s*)?", e)
                if not em:
                    raise _unparsed(e)
                v = constants[em[1]] = int(em[2]) if em[2] else v + 1
        else:
            ret = re.sub(r"\s*\*", "*", " ".join(m["ret"].split()))
            restype = {"void": None, "const char*": ctypes.c_char_p}.get(ret, False)
            if restype is False:
                restype = _ctype(ret.rstrip("*"), ret.count("*"), m[0])
            params = m["params"].strip()
            functions[m["fn"]] = (restype, [] if params == "void" else [_param(p) for p in params.split(",")])
    return functions, structs, constants


FUNCTIONS, STRUCTS, CONSTANTS = parse_header()


def header_symbols():
    """Every function name declared in include/bsed.h."""
    return sorted(FUNCTIONS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BsedError(f"{LIB_PATH} is missing: build it with csrc/build.sh "
                            "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in FUNCTIONS.items():
            fn = getattr(L, name)  # AttributeError = header/library mismatch: fail loudly
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise BsedError(f"{what} failed ({rc}): {lib().bsed_last_error().decode()}")


def _require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise BsedError("bsed_amd needs an MI355X (torch.cuda.is_available() is False); there is no CPU fallback")


def ptr(t, dtype=None):
    """Device pointer of a contiguous CUDA(HIP) tensor, or NULL for None."""
    import torch
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise BsedError("expected a GPU tensor")
    if t.device.index != torch._C._cuda_getDevice():
        # launches go to the CURRENT device's stream (stream() below): a tensor of another GPU would be dereferenced
        # by a kernel running on the wrong device
        raise BsedError(f"tensor lives on cuda:{t.device.index} but the current device is "
                        f"cuda:{torch._C._cuda_getDevice()}: wrap the call in torch.cuda.device(...)")
    if not t.is_contiguous():
        raise BsedError("expected a contiguous tensor")
    want = torch.float32 if dtype is None else dtype
    if t.dtype != want:
        raise BsedError(f"expected dtype {want}, got {t.dtype}")
    return ctypes.c_void_p(t.data_ptr())


_raw_stream = None


def stream():
    """torch's current stream on the current device as a hipStream_t.  (torch.cuda.current_stream() builds a Python
    Stream object: ~8 us per call, a quarter of the host time of a launch-bound small-batch step.)"""
    global _raw_stream
    import torch
    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if _raw_stream:
        return ctypes.c_void_p(_raw_stream(torch._C._cuda_getDevice()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Per-launch timing hook (bench.py's roofline leg): ``timer`` is an ops.KernelTimer or None.  A wrapper that knows the
# algorithmic work of its launch announces it through ``pending`` = (key, flops, bytes) right before ``call``; launches
# nobody announced are recorded under their entry-point name with zero work (small glue kernels).
timer = None
pending = None


def call(name, *args):
    """Call an int-returning entry point and raise on a nonzero return; the header's argtypes convert the arguments."""
    global pending
    fn = getattr(lib(), name)
    if timer is None:
        check(fn(*args), name)
        return
    meta, pending = pending, None
    key, flops, nbytes = meta if meta is not None else ((name, ""), 0.0, 0.0)
    timer.launch(key, flops, lambda: check(fn(*args), name), nbytes)


c_int = ctypes.c_int
c_float = ctypes.c_float
