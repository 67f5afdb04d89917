"""What the all-pairs measures of an embedding share on the host (``domain_gap``, ``tsne``, ``svc``): the check of a tensor
and of the (N, D) point matrix the kernels read, the check that a dense (N, N) float32 matrix fits the device, the two
domains put together as one point matrix, and the embeddings themselves -- from a model's loaders (``embed``,
``embed_two``) or from the dumps of ``get_predictions(saved_feature_dir=...)`` (``load_embedded_features``).  It lives
beside the ``evaluation`` package; what it needs from the package is imported inside the function that uses it."""
import os
import re

import numpy as np
import torch

from . import _lib as L
from ._lib import BsedError


def gpu_tensor(x, who, name, dtype, dim):
    """``x`` as it is, when it is a ``dim``-dimensional ``dtype`` tensor on the current GPU; a ``BsedError`` otherwise"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise BsedError(f"{who}: {name} must be a GPU tensor (there is no CPU path)")
    if x.dtype != dtype or x.dim() != dim:
        raise BsedError(f"{who}: {name} must be a {dim}-dimensional {dtype} tensor, got {tuple(x.shape)} {x.dtype}")
    if x.device.index != torch._C._cuda_getDevice():
        raise BsedError(f"{who}: {name} lives on cuda:{x.device.index} but the current device is "
                        f"cuda:{torch._C._cuda_getDevice()}: wrap the call in torch.cuda.device(...)")
    return x


def gpu_matrix(x, who, name="x", min_n=1, max_n=None, cols=None):
    """``gpu_tensor`` for a float32 (N, ``cols`` or any D >= 1) matrix of ``min_n`` to ``max_n`` (None: any number of)
    rows; nothing is copied"""
    x = gpu_tensor(x, who, name, torch.float32, 2)
    N, D = x.shape
    if D < 1 or (cols is not None and D != cols) or N < min_n or (max_n is not None and N > max_n):
        raise BsedError(f"{who}: {name} must be (N, {cols or 'D'}) with D >= 1 and {min_n} to {max_n or 'any number of'} "
                        f"points, got {tuple(x.shape)}")
    return x


def gpu_points(x, who, min_n=1, max_n=None):
    """The point matrix of a kernel: ``gpu_matrix``, made unit-stride along D with rows at least D apart (a copy only
    when it is not) -> ``(x, pitch)``, the pitch in elements.  The stride of the only row of a (1, D) tensor means
    nothing and may be anything: D is passed for it."""
    x = gpu_matrix(x, who, "x", min_n, max_n)
    N, D = x.shape
    if x.stride(1) != 1 or (N > 1 and x.stride(0) < D):
        x = x.contiguous()
    return x, (x.stride(0) if N > 1 else D)


def check_dense_fits(n, device, who, what):
    """raises when the dense (n, n) float32 matrix ``what`` does not fit the free memory of ``device`` (torch's cache
    counted as free); the message names the bytes"""
    free, _total = torch.cuda.mem_get_info(device)
    free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)   # what torch's cache can hand out
    need = 4 * int(n) * int(n)
    if need > free:
        raise BsedError(f"{who}: the {what} of {n} points need {need} bytes of device memory, {free} are free; "
                        "there is no host fallback: draw fewer points (max_points)")


def two_domains(synth, real, who):
    """two (n, D) sets of points (arrays or tensors) -> ``(x, n_synth, n_real)``: the float32 GPU matrix of both, synth
    first"""
    L._require_gpu()
    s, r = (torch.as_tensor(v).float().cuda() for v in (synth, real))
    if s.dim() != 2 or r.dim() != 2 or s.shape[1] != r.shape[1] or s.shape[0] < 1 or r.shape[0] < 1:
        raise BsedError(f"{who}: two non-empty (n, D) sets of the same D, got {tuple(s.shape)} and {tuple(r.shape)}")
    return torch.cat([s, r], dim=0), s.shape[0], r.shape[0]


def _points(features, level):
    if level not in ("clip", "frame"):
        raise BsedError(f"level must be 'clip' or 'frame', got {level!r}")
    if features.ndim != 3:
        raise BsedError(f"embedded features must be (B, T', F), got {tuple(features.shape)}")
    return features.reshape(features.shape[0], -1) if level == "clip" else features.reshape(-1, features.shape[2])


def embed(model, dataloader, predictor, fpn=False, level="clip", max_points=None, seed=0):
    """The encoder's second output (what ``saved_feature_dir`` dumps) of every batch of ``dataloader`` in eval mode ->
    (n, D) float32 GPU tensor; the features never leave the GPU.  ``level="clip"``: one point per clip, its (T', F)
    features flattened (src/visualize.py:153); ``level="frame"``: one point per frame, D = F.  ``max_points``: that many
    points drawn without replacement by a torch generator seeded with ``seed``, kept in their order."""
    from .evaluation._common import _batches, _check_form, _eval_mode, _forward
    _check_form("embed", predictor, fpn)
    out = []
    with _eval_mode(model, predictor):
        for x, _target, _paths, _names, _folders in _batches(dataloader):
            features = _forward(model, predictor, fpn, x, features=True)[2]
            if features is None:
                raise BsedError("embed: the forward handed out no features (a self-contained model, predictor=None, "
                                "does not return the encoder's output)")
            out.append(_points(features.float(), level))
    if not out:
        raise BsedError("embed: the loader is empty")
    points = torch.cat(out, dim=0)
    if max_points is not None and points.shape[0] > int(max_points):
        gen = torch.Generator().manual_seed(int(seed))
        keep = torch.randperm(points.shape[0], generator=gen)[:int(max_points)].sort().values
        points = points[keep.to(points.device)]
    return points.contiguous()


def embed_two(model, synth_loader, real_loader, predictor, fpn=False, level="clip", max_points=None, seed=0):
    """``embed`` of the two loaders, each with the same ``max_points`` and ``seed`` -> ``(synth, real)``"""
    return tuple(embed(model, loader, predictor, fpn, level, max_points, seed) for loader in (synth_loader, real_loader))


def load_embedded_features(folder, level="clip"):
    """the ``<i>.npy`` batches that ``get_predictions(saved_feature_dir=folder)`` wrote -> (n, D) float32 numpy array,
    read in the NUMERIC order of ``i`` (0, 1, 2, ..., 10: the order the batches were made in).  The reference
    concatenates them in ``os.listdir`` order (src/visualize.py:146-153), which is arbitrary; the measures here do not
    depend on the order of the points, only ``nn_index`` refers to it."""
    names = [n for n in os.listdir(folder) if re.fullmatch(r"\d+\.npy", n)]
    if not names:
        raise BsedError(f"load_embedded_features: no <i>.npy file in {folder}")
    names.sort(key=lambda n: int(n[:-4]))
    return np.concatenate([_points(np.load(os.path.join(folder, n)), level) for n in names], axis=0).astype(np.float32)
