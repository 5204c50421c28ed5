"""Rows of a FROZEN spot classifier, kept per array across epochs (new; opt-in through `GridNet.enable_f_cache`).

The tutorials' grid recipe trains only the corrector g: f is frozen, `patch_classifier.eval()` is forced in both phases
(gridnext/training.py:126 of the reference) and still `model(inputs)` (:146) evaluates f on every array in every epoch - one
78 x 64 array of 128-px patches is ~57 ms of f against ~0.25 ms of g.  The reference's authors work around it by hand
(notebooks/register_concat.ipynb cells 1-4: save `patch_predictions` to .npy, train a second model on the maps).  Here the
model does it: a frozen eval-mode f maps equal bytes to equal rows, so `FrozenRowCache` keeps each array's rows
[spots_per_array, f_dim] on the device under a 128-bit fingerprint of the array's bytes (csrc/fingerprint.hip,
include/gridnext_hip.h "content fingerprint") and hands out copies when the same bytes come back.

  * the key is (fingerprint, bytes per array, dtype, per-array shape); nothing about where the array sits in memory, which
    loader produced it or in which order - a shuffling loader and a pinned-ring prefetcher hit as well as resident tensors;
  * the cache belongs to ONE state of ONE classifier: `classifier_state(f)` lists the (`_version`, `data_ptr()`) of every parameter
    and buffer (the scheme of `DenseNet._key` and `functional._frozen_affine_plan`) and, for a DenseNet, every switch that
    selects its arithmetic.  A different token empties the cache before anything is looked up;
  * one lookup is one fingerprint launch over the batch's arrays and ONE read-back of 16 bytes per array - a host
    synchronisation per step, which is what lets the host decide not to enqueue f at all;
  * the byte budget is a cap, not a policy: when the next array's rows do not fit they are simply not kept (an epoch walks
    every array once, so evicting would only trade one miss for another).

Whether a call may be served at all (device, contiguity, no stream capture, eval mode, nothing requiring grad) is the
model's decision (`GridNet._f_cache_ok`); calls it turns away are counted in `bypassed`.
"""
import torch

from . import _lib as L

# DenseNet attributes that select the arithmetic of its eval forward (densenet.py: __init__): part of the state token
_DENSENET_SWITCHES = ('mfma', 'split_conv1', 'split_conv2', 'split_wgrad', 'winograd', 'skip_empty', 'two_ranges', 'f16_buffers',
                      'f16_stem', 'f16_fused', 'f16_fused_transitions', 'f16_fused_conv2_backward', 'atonce', 'input_norm',
                      'input_resize', 'input_crop')


def device_fingerprint(src, n_seg):
    """[(lane0, lane1)] * n_seg: the fingerprints of the `n_seg` equal, back-to-back parts of the contiguous device tensor
    `src` (gnx_fingerprint128_batch on the current stream, then one read-back)."""
    if not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("device_fingerprint needs a contiguous tensor on a HIP device; there is no CPU path")
    if n_seg == 0:
        return []
    total = src.numel() * src.element_size()
    if total % n_seg:
        raise ValueError("%d bytes do not divide into %d segments" % (total, n_seg))
    seg_bytes = total // n_seg
    out = torch.empty((n_seg, 2), device=src.device, dtype=torch.int64)
    ws_bytes = L.query('gnx_fingerprint128_batch_workspace', seg_bytes, n_seg)
    ws = torch.empty(ws_bytes // 8, device=src.device, dtype=torch.int64) if ws_bytes else None
    L.call('gnx_fingerprint128_batch', src.data_ptr(), seg_bytes, n_seg, L.ptr(out, torch.int64), L.ptr(ws, torch.int64), L.stream())
    return [(a & 0xFFFFFFFFFFFFFFFF, b & 0xFFFFFFFFFFFFFFFF) for a, b in out.tolist()]      # (.tolist(): the step's host sync)


def _walk(module, out):
    out.append(module)
    for child in module._modules.values():
        if child is not None:
            _walk(child, out)
    return out


def classifier_state(classifier):
    """(token, frozen) of `classifier` in ONE walk of its module tree (this runs every step, and `Module.parameters()` /
    `.buffers()` / `.modules()` each walk a DenseNet-121's 430 modules building their dotted names: 2.7 ms together
    against 0.9 ms this way, on one host).
    token: what cached rows depend on besides the input - every parameter and buffer by (`_version`, `data_ptr()`): in-place
    edits, optimizer steps, `load_state_dict` and `.to()` all change it - and, for a `gridnext_amd.DenseNet`, its cache
    epoch (`invalidate_cache`: writes that bump no version) and its arithmetic switches.
    frozen: every module in eval mode and no parameter requiring grad."""
    from .densenet import DenseNet
    tensors, frozen = [], True
    for m in _walk(classifier, []):
        frozen = frozen and not m.training
        for p in m._parameters.values():
            if p is not None:
                tensors.append(p)
                frozen = frozen and not p.requires_grad
        for b in m._buffers.values():
            if b is not None:
                tensors.append(b)
    if isinstance(classifier, DenseNet):
        switches = tuple((n, repr(getattr(classifier, n, None))) for n in _DENSENET_SWITCHES)
        return (id(classifier), classifier._key(tensors), switches), frozen
    return (id(classifier), tuple((t._version, t.data_ptr()) for t in tensors)), frozen


def state_token(classifier):
    return classifier_state(classifier)[0]


class FrozenRowCache:
    """(fingerprint, bytes, dtype, shape) of an array -> the frozen classifier's rows [spots_per_array, f_dim] for it.

    `fingerprint(src, n_seg) -> [(lane0, lane1)] * n_seg` is injected (default: `device_fingerprint`), so the bookkeeping
    runs anywhere.  `hits` / `misses` count arrays, `bypassed` counts calls the owner did not send through the cache."""

    def __init__(self, max_bytes=1 << 30, fingerprint=None):
        self.max_bytes = int(max_bytes)
        self.fingerprint = device_fingerprint if fingerprint is None else fingerprint
        self.hits = self.misses = self.bypassed = 0
        self.clear()

    def clear(self):
        """Drop every entry (and the state token they belonged to); the counters keep counting."""
        self._rows = {}
        self._token = None
        self.bytes = 0

    def __len__(self):
        return len(self._rows)

    def bypass(self):
        self.bypassed += 1

    def fetch(self, token, src, n_arrays, compute):
        """Rows [n_arrays * spots_per_array, f_dim] of the `n_arrays` equal parts of the contiguous tensor `src`, in order.
        `token`: the classifier's `state_token` now.  `compute(idx)`: the rows of the arrays `idx` (ascending positions in
        the batch; None = all of them, the batch as it stands), evaluated together in that order - called at most once, for
        the arrays the cache does not hold.  The result never aliases cached storage."""
        if token != self._token:
            self.clear()
            self._token = token
        seg_bytes = src.numel() * src.element_size() // max(n_arrays, 1)
        shape = tuple(src.shape[1:]) if src.dim() and src.shape[0] == n_arrays else (src.numel() // max(n_arrays, 1),)
        keys = [(fp, seg_bytes, src.dtype, shape) for fp in self.fingerprint(src, n_arrays)]
        assert len(keys) == n_arrays
        found = [self._rows.get(k) for k in keys]
        missed = [i for i, r in enumerate(found) if r is None]
        self.hits += n_arrays - len(missed)
        self.misses += len(missed)
        if not missed:
            return torch.cat(found, 0) if n_arrays != 1 else found[0].clone()
        fresh = compute(None if len(missed) == n_arrays else missed)
        per = fresh.shape[0] // len(missed)
        assert per * len(missed) == fresh.shape[0], "compute() returned %d rows for %d arrays" % (fresh.shape[0], len(missed))
        for k, i in enumerate(missed):
            part = fresh.narrow(0, k * per, per)
            nbytes = part.numel() * part.element_size()
            if keys[i] not in self._rows and self.bytes + nbytes <= self.max_bytes:
                self._rows[keys[i]] = part.detach().clone()          # the cache's own storage: `fresh` goes to the caller
                self.bytes += nbytes
        if len(missed) == n_arrays:
            return fresh
        out = fresh.new_empty((n_arrays * per,) + tuple(fresh.shape[1:]))
        k = 0
        for i in range(n_arrays):
            if found[i] is None:
                out.narrow(0, i * per, per).copy_(fresh.narrow(0, k * per, per))
                k += 1
            else:
                out.narrow(0, i * per, per).copy_(found[i])
        return out
