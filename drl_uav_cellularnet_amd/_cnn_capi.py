"""ctypes binding of libuavcnn.so (include/uavcnn.h, ABI 1): thin launch wrappers for cnn_agent.py (current torch stream, no allocation
beyond outputs and workspaces).  A CUDA tensor with no library is an error, not a silent PyTorch fallback."""
import ctypes as C
import os

import torch

from . import build as _build

EXPORTS = ("uavcnn_abi_version", "uavcnn_last_error", "uavcnn_conv1_from_idx_f32", "uavcnn_conv5_f32", "uavcnn_conv5_wgrad_workspace_bytes",
           "uavcnn_conv5_wgrad_f32", "uavcnn_conv1_wgrad_workspace_bytes", "uavcnn_conv1_wgrad_from_idx_f32", "uavcnn_dense_fwd_workspace_bytes",
           "uavcnn_dense_fwd_f32", "uavcnn_dense_dx_f32", "uavcnn_dense_wgrad_f32")
ABI_VERSION = 1
KSIZE, FILTERS, DENSE = 5, 10, 100

_lib = None
_P, _I64, _I32, _SZ = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t


class UavCnnError(RuntimeError):
    pass


def lib_path():
    return os.environ.get("UAVCNN_LIB") or _build.CNN_LIB


# per-launch timing for tools/bench_cnn.py: profile_begin() makes load() hand out a proxy that brackets every launch with HIP events
_prof = None


class _ProfiledLib:
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith("_f32"):
            return fn

        def timed(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            if _prof is not None:
                _prof.setdefault(name, []).append((e0, e1))
            return rc
        return timed


def profile_begin():
    global _prof
    load()
    _prof = {}


def profile_end():
    """-> {entry point: [ms, ...]} for every launch since profile_begin() (synchronises the device)."""
    global _prof
    torch.cuda.synchronize()
    out = {k: [a.elapsed_time(b) for a, b in v] for k, v in (_prof or {}).items()}
    _prof = None
    return out


def load():
    global _lib
    if _lib is not None:
        return _ProfiledLib(_lib) if _prof is not None else _lib
    path = lib_path()
    if not os.path.isfile(path):
        raise UavCnnError("%s not found: run `python -m drl_uav_cellularnet_amd.build` (there is no fallback for CUDA tensors)" % path)
    lib = C.CDLL(path)
    lib.uavcnn_abi_version.restype = C.c_int
    lib.uavcnn_last_error.restype = C.c_char_p
    sig = {
        "uavcnn_conv1_from_idx_f32": [_P, _I64, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P],
        "uavcnn_conv5_f32": [_P, _I64, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P],
        "uavcnn_conv5_wgrad_f32": [_P, _P, _I64, _I32, _I32, _I32, _P, _P, _I32, _P, _SZ, _P],
        "uavcnn_conv1_wgrad_from_idx_f32": [_P, _I64, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _I32, _P, _SZ, _P],
        "uavcnn_dense_fwd_f32": [_P, _I64, _I64, _I32, _P, _P, _P, _P, _SZ, _P],
        "uavcnn_dense_dx_f32": [_P, _P, _P, _I64, _I64, _I32, _P, _P],
        "uavcnn_dense_wgrad_f32": [_P, _P, _I64, _I64, _I32, _P, _I32, _P],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args
    for name, args in (("uavcnn_conv5_wgrad_workspace_bytes", [_I64, _I32]), ("uavcnn_conv1_wgrad_workspace_bytes", [_I64, _I32]),
                       ("uavcnn_dense_fwd_workspace_bytes", [_I64, _I64])):
        getattr(lib, name).restype = _SZ
        getattr(lib, name).argtypes = args
    if lib.uavcnn_abi_version() != ABI_VERSION:
        raise UavCnnError("libuavcnn.so ABI version mismatch")
    _lib = lib
    return lib


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check(rc, what):
    if rc != 0:
        raise UavCnnError("%s: %s" % (what, load().uavcnn_last_error().decode()))


def _f32(what, *tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise UavCnnError("%s: operands must be contiguous float32 CUDA tensors" % what)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise UavCnnError("%s: operands on different devices" % what)


def _idx(idx, what):
    if idx.dtype != torch.int64 or idx.dim() != 2 or not idx.is_contiguous() or not idx.is_cuda:
        raise UavCnnError("%s: idx must be a contiguous int64 [M, K] CUDA tensor" % what)


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def conv1_from_idx(idx, n_bs, grid, k_a, b_a, y_a, k_c=None, b_c=None, y_c=None):
    """y = relu(conv1(count map of idx) + b) for one or both trunks; y_* [M, G-4, G-4, 10]."""
    _idx(idx, "conv1_from_idx")
    _f32("conv1_from_idx", k_a, b_a, y_a, k_c, b_c, y_c)
    M, K = idx.shape
    for y in (y_a, y_c):
        if y is not None and tuple(y.shape) != (M, grid - 4, grid - 4, FILTERS):
            raise UavCnnError("conv1_from_idx: outputs must be [M, G-4, G-4, 10]")
    with torch.cuda.device(idx.device):
        rc = load().uavcnn_conv1_from_idx_f32(_ptr(idx), M, K, int(n_bs), int(grid), KSIZE, FILTERS, _ptr(k_a), _ptr(b_a), _ptr(y_a), _ptr(k_c),
                                              _ptr(b_c), _ptr(y_c), _stream(idx.device))
    _check(rc, "uavcnn_conv1_from_idx_f32")
    return y_a


def conv5(x, w, y, pad=0, bias=None, mask=None):
    """y = relu(corr(x, w) + bias) (forward) or corr(x, w) * (mask > 0) (dX, pad 4, flipped w); NHWC [M, S, S, 10]."""
    _f32("conv5", x, w, y, bias, mask)
    M, S = x.shape[0], x.shape[1]
    So = S - 4 + 2 * pad
    if tuple(x.shape) != (M, S, S, FILTERS) or tuple(y.shape) != (M, So, So, FILTERS) or (mask is not None and mask.shape != y.shape):
        raise UavCnnError("conv5: shapes do not agree: x %s, y %s, pad %d" % (tuple(x.shape), tuple(y.shape), pad))
    with torch.cuda.device(x.device):
        rc = load().uavcnn_conv5_f32(_ptr(x), M, S, int(pad), KSIZE, FILTERS, _ptr(w), _ptr(bias), _ptr(mask), _ptr(y), _stream(x.device))
    _check(rc, "uavcnn_conv5_f32")
    return y


def conv5_wgrad_workspace(m_rows, s_in, device):
    return workspace(load().uavcnn_conv5_wgrad_workspace_bytes(int(m_rows), int(s_in)), device)


def conv5_wgrad(x, dy, dw, db, ws, accumulate=False):
    _f32("conv5_wgrad", x, dy, dw, db)
    M, S = x.shape[0], x.shape[1]
    if tuple(dy.shape) != (M, S - 4, S - 4, FILTERS):
        raise UavCnnError("conv5_wgrad: dy must be [M, S-4, S-4, 10]")
    with torch.cuda.device(x.device):
        rc = load().uavcnn_conv5_wgrad_f32(_ptr(x), _ptr(dy), M, S, KSIZE, FILTERS, _ptr(dw), _ptr(db), 1 if accumulate else 0, _ptr(ws),
                                           ws.numel(), _stream(x.device))
    _check(rc, "uavcnn_conv5_wgrad_f32")


def conv1_wgrad_workspace(m_rows, n_bs, device):
    return workspace(load().uavcnn_conv1_wgrad_workspace_bytes(int(m_rows), int(n_bs)), device)


def conv1_wgrad(idx, n_bs, grid, dy, dk, db, ws, accumulate=False):
    _idx(idx, "conv1_wgrad")
    _f32("conv1_wgrad", dy, dk, db)
    M, K = idx.shape
    if tuple(dy.shape) != (M, grid - 4, grid - 4, FILTERS):
        raise UavCnnError("conv1_wgrad: dy must be [M, G-4, G-4, 10]")
    with torch.cuda.device(idx.device):
        rc = load().uavcnn_conv1_wgrad_from_idx_f32(_ptr(idx), M, K, int(n_bs), int(grid), KSIZE, FILTERS, _ptr(dy), _ptr(dk), _ptr(db),
                                                    1 if accumulate else 0, _ptr(ws), ws.numel(), _stream(idx.device))
    _check(rc, "uavcnn_conv1_wgrad_from_idx_f32")


def dense_fwd_workspace(m_rows, d, device):
    return workspace(load().uavcnn_dense_fwd_workspace_bytes(int(m_rows), int(d)), device)


def dense_fwd(flat, w, bias, h, ws):
    """h = relu6(flat @ w + bias); flat [M, D], w [D, 100]."""
    _f32("dense_fwd", flat, w, bias, h)
    M, D = flat.shape
    if tuple(w.shape) != (D, DENSE) or tuple(h.shape) != (M, DENSE):
        raise UavCnnError("dense_fwd: shapes do not agree")
    with torch.cuda.device(flat.device):
        rc = load().uavcnn_dense_fwd_f32(_ptr(flat), M, D, DENSE, _ptr(w), _ptr(bias), _ptr(h), _ptr(ws), ws.numel(), _stream(flat.device))
    _check(rc, "uavcnn_dense_fwd_f32")
    return h


def dense_dx(dh, w, flat, dflat):
    """dflat = (dh @ w.T) * (flat > 0)."""
    _f32("dense_dx", dh, w, flat, dflat)
    M, D = flat.shape
    if tuple(w.shape) != (D, DENSE) or tuple(dh.shape) != (M, DENSE) or dflat.shape != flat.shape:
        raise UavCnnError("dense_dx: shapes do not agree")
    with torch.cuda.device(flat.device):
        rc = load().uavcnn_dense_dx_f32(_ptr(dh), _ptr(w), _ptr(flat), M, D, DENSE, _ptr(dflat), _stream(flat.device))
    _check(rc, "uavcnn_dense_dx_f32")
    return dflat


def dense_wgrad(flat, dh, dw, accumulate=False):
    """dw (+)= flat.T @ dh, [D, 100]."""
    _f32("dense_wgrad", flat, dh, dw)
    M, D = flat.shape
    if tuple(dw.shape) != (D, DENSE) or tuple(dh.shape) != (M, DENSE):
        raise UavCnnError("dense_wgrad: shapes do not agree")
    with torch.cuda.device(flat.device):
        rc = load().uavcnn_dense_wgrad_f32(_ptr(flat), _ptr(dh), M, D, DENSE, _ptr(dw), 1 if accumulate else 0, _stream(flat.device))
    _check(rc, "uavcnn_dense_wgrad_f32")
    return dw
