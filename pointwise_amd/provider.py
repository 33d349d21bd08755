"""Device-resident batch provider: one fused launch per batch (include/conv3p.h: conv3p_provider_batch_f32).

The reference feeds its models from host-side providers,
    DataConsumer of modelnet_provider.py:114-219           (ModelNet40: slice to num_points, shuffle, rotate, jitter,
                                                            optional sort, one uint8 label per cloud)
    DataConsumer of scene_seg/s3dis_provider.py:15-118,
                    scene_seg/scenenn_provider.py:14-105   (rooms: epoch permutation, optional sort of rows and per-point
                                                            labels, points = rows[:, :, 0:3])
with numpy loops per cloud.  Here the data set -- arrays already in memory; reading HDF5 is not this module's job --
is uploaded once, and a batch is assembled from it by ONE kernel launch: index, slice, rotate, jitter, sort, the
points / input split and the label cast.  The random draws are the device's (Philox4x32-10, a function of seed, step,
sample and source row: pointwise_amd/csrc/conv3p_provider.hpp), so an epoch is reproducible from (seed, epoch) alone
and does not depend on how the batch is sharded.  sort_method is the providers' own argument
(modelnet_provider.py:202-208): "xyz" or "morton", the latter in the order include/conv3p.h defines (the reference takes
its codes from the third-party `libpluie`, which nobody has).

    assemble_batch   the call, on tensors
    BatchProvider    the reference providers' interface (next_epoch, has_next_batch, next_batch,
                     get_batch_point_cloud, num_batches, num_points, num_channels) over it

A sorted batch is one launch for clouds of up to 8192 points.  wide_sort=True routes a sorted batch to
conv3p_provider_batch_wide_f32 instead: several launches, a cloud spread over many workgroups, up to 65536 points, the
same bits wherever both apply (pointwise_amd/csrc/conv3p_sort_wide.hpp).
"""
import numpy as np
import torch

from . import _lib
from . import prestep
from ._host import _LABEL_DTYPES, Conv3pInvalidArgument, _call, _ptr, _require, _require_tensor, _stream
from .prestep import SORT_METHODS


def _check_sort_method(sort_method):
    """The reference prints a message and feeds unsorted clouds when it does not know the method; here it is an error,
    raised before anything touches the device (prestep's check) -> the method."""
    prestep._check_sort_method(sort_method, tuple(SORT_METHODS))
    return sort_method


def _sort_flags(sort_cloud, sort_method):
    """sort_method is inert while sort_cloud is false, as in the reference."""
    if not sort_cloud:
        return 0
    return _lib.PROVIDER_SORT | (_lib.PROVIDER_MORTON if sort_method == "morton" else 0)


def _workspace_bytes(lib, wide):
    return lib.conv3p_provider_wide_workspace_bytes if wide else lib.conv3p_provider_workspace_bytes


class BatchBuffers:
    """The output tensors of one batch and the call's scratch: points (B, N, 3), input (B, N, K), labels int32 (B) or
    (B, N), bad_index int32 (), and -- with randoms -- cos_sin (B, 2), noise (B, N, 3) float64, order int32 (B, N)."""

    def __init__(self, B, N, K, per_point, device, sort_cloud=False, randoms=False, sort_method="xyz", wide_sort=False):
        self.shape = (B, N, K, bool(per_point))
        self.points = torch.empty((B, N, 3), dtype=torch.float32, device=device)
        self.input = torch.empty((B, N, K), dtype=torch.float32, device=device)
        self.labels = torch.empty((B, N) if per_point else (B,), dtype=torch.int32, device=device)
        self.bad_index = torch.zeros((), dtype=torch.int32, device=device)
        flags = _sort_flags(sort_cloud, _check_sort_method(sort_method))
        nbytes = _workspace_bytes(_lib.load(), wide_sort and sort_cloud)(B, N, flags)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None
        self.cos_sin = self.noise = self.order = None
        if randoms:
            self.cos_sin = torch.empty((B, 2), dtype=torch.float64, device=device)
            self.noise = torch.empty((B, N, 3), dtype=torch.float64, device=device)
            self.order = torch.empty((B, N), dtype=torch.int32, device=device)


def assemble_batch(data, labels, batch_size, num_points=None, perm=None, start=0, rotate=False, jitter=False, sigma=0.01,
                   clip=0.05, sort_cloud=False, seed=0, step=0, cos_sin=None, noise=None, out=None, return_randoms=False,
                   sort_method="xyz", wide_sort=False):
    """One batch from a resident data set, in one launch.

    data float32 (S, Nsrc, K) with xyz first; labels uint8 / int32 / int64, (S,) or (S, Nsrc); cloud b is sample
    perm[start + b] (perm int32 on the device; None: start + b) cut to its first num_points rows (default Nsrc).
    rotate / jitter / sort_cloud / sort_method ("xyz" or "morton"; inert without sort_cloud; anything else: ValueError):
    modelnet_provider.py:196-208; cos_sin (B, 2) and noise (B, N, 3), float64 device tensors, replace the draws of
    (seed, step).  out: a BatchBuffers to write into (default: fresh tensors).
    -> (points (B, N, 3), input (B, N, K), labels int32, bad_index) and, with return_randoms, a dict of cos_sin, noise
    (source-row order) and order.  wide_sort (inert without sort_cloud): the sort spread over many workgroups, in several
    launches, for num_points up to 65536 instead of 8192; the same bits.  bad_index is an int32 device scalar: the number
    of clouds whose sample index was outside [0, S) -- their rows are 0 and their labels -1; it is not synchronised on
    here."""
    _check_sort_method(sort_method)
    lib = _lib.load()
    _require(isinstance(data, torch.Tensor) and data.dim() == 3 and data.dtype == torch.float32 and data.shape[2] >= 3,
             "data must be a float32 (S, Nsrc, K >= 3) tensor, xyz first")
    _require(isinstance(labels, torch.Tensor) and labels.dtype in _LABEL_DTYPES, "labels must be uint8, int32 or int64")
    dev = data.device
    S, Nsrc, K = data.shape
    _require(S <= 2 ** 31 - 1, "at most 2^31 - 1 samples")
    _require(labels.device == dev, "labels must be on the data's device")
    _require(tuple(labels.shape) in ((S,), (S, Nsrc)), "labels must be (S,) or (S, Nsrc)")
    per_point = labels.dim() == 2
    _require(data.is_contiguous() and labels.is_contiguous(), "data and labels must be contiguous")
    B = int(batch_size)
    N = Nsrc if num_points is None else int(num_points)
    _require(B >= 0 and 0 <= N <= Nsrc, "batch_size >= 0 and 0 <= num_points <= Nsrc expected")
    start = int(start)
    _require(start >= 0, "start must not be negative")
    if perm is not None:
        _require_tensor(perm, "perm must be a contiguous int32 vector on the data's device", torch.int32, dev=dev, ndim=1)
        _require(start + B <= perm.numel(), "batch_size + start reaches past perm")
    else:
        _require(start + B <= 2 ** 31 - 1, "start out of range")
    _require(0 <= int(seed) < 2 ** 64 and 0 <= int(step) < 2 ** 64, "seed and step must fit 64 unsigned bits")
    if jitter:
        _require(clip > 0, "clip must be positive")                      # assert(clip > 0), modelnet_provider.py:72
        _require(sigma >= 0, "sigma must not be negative")
    for name, t, on, shape in (("cos_sin", cos_sin, rotate, (B, 2)), ("noise", noise, jitter, (B, N, 3))):
        if t is None:
            continue
        _require(on, "%s given without the augmentation it belongs to" % name)
        _require_tensor(t, "%s must be a contiguous float64 %s tensor on the data's device" % (name, shape), torch.float64,
                        shape, dev)
    _require(dev.type == "cuda", "data must live on a HIP device (there is no CPU path)")   # after every other check
    if out is None:
        out = BatchBuffers(B, N, K, per_point, dev, sort_cloud, return_randoms, sort_method, wide_sort)
    else:
        _require(isinstance(out, BatchBuffers) and out.shape == (B, N, K, per_point) and out.points.device == dev,
                 "out was made for another batch shape")
        _require(not return_randoms or out.noise is not None, "out has no buffers for the randoms")
    flags = ((_lib.PROVIDER_ROTATE if rotate else 0) | (_lib.PROVIDER_JITTER if jitter else 0)
             | _sort_flags(sort_cloud, sort_method))
    wide = bool(wide_sort and sort_cloud)
    need = _workspace_bytes(lib, wide)(B, N, flags)
    ws = out.workspace
    if need and (ws is None or ws.numel() < need):
        ws = out.workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    rnd = return_randoms
    if B * N == 0:                       # nothing is launched, so nothing is written
        out.bad_index.zero_()
        out.labels.fill_(-1)
        res = (out.points, out.input, out.labels, out.bad_index)
        return res + ({"cos_sin": out.cos_sin, "noise": out.noise, "order": out.order},) if return_randoms else res
    with torch.cuda.device(dev):
        _call(lib.conv3p_provider_batch_wide_f32 if wide else lib.conv3p_provider_batch_f32,
              _ptr(data), _ptr(labels), S, Nsrc, K, _LABEL_DTYPES[labels.dtype],
              int(per_point), _ptr(perm), perm.numel() if perm is not None else 0,
              start, B, N, flags, float(sigma), float(clip), int(seed), int(step), _ptr(cos_sin), _ptr(noise),
              _ptr(out.points), _ptr(out.input), _ptr(out.labels),
              _ptr(out.cos_sin) if rnd else None, _ptr(out.noise) if rnd else None, _ptr(out.order) if rnd else None,
              out.bad_index.data_ptr(), _ptr(ws, need), ws.numel() if need else 0,
              _stream(dev))
    res = (out.points, out.input, out.labels, out.bad_index)
    if return_randoms:
        res += ({"cos_sin": out.cos_sin, "noise": out.noise, "order": out.order},)
    return res


class BatchProvider:
    """The reference providers' DataConsumer over a data set resident on the device.

    data (S, Nsrc, K) float32 and labels (S,) or (S, Nsrc), numpy arrays or tensors, are uploaded once.
    training=True reshuffles per epoch -- np.random.default_rng([seed, epoch]).permutation(S), uploaded once per epoch
    (next_epoch of the scene providers; shuffle_data of modelnet_provider.py:175) -- and training=False keeps the
    identity order and never augments (`test` there).  rotate / jitter default to `training` for xyz-only data (the
    ModelNet provider) and to False otherwise (the scene providers never augment).  The draws of batch `cur_batch` of
    epoch `epoch` are those of step = epoch * num_batches + cur_batch.

    get_batch_point_cloud() -> (points, input, labels int32); the tensors alternate between two buffer sets, so a batch
    stays valid while the next one is assembled.  bad_index (int32 device scalar) belongs to the last batch.
    sort_method ("xyz" or "morton") is a constructor setting like sort_cloud, not state: state_dict does not carry it.
    Neither is wide_sort (assemble_batch's: sorted batches of clouds of up to 65536 points; inert without sort_cloud)."""

    def __init__(self, data, labels, batch_size, num_points=None, training=True, rotate=None, jitter=None,
                 sort_cloud=False, seed=0, device="cuda:0", sort_method="xyz", wide_sort=False):
        self.sort_method = _check_sort_method(sort_method)
        self.wide_sort = bool(wide_sort)
        self.device = torch.device(device)
        as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, order="C"))   # a copy: uploaded once
        data, labels = as_t(data), as_t(labels)
        _require(data.dim() == 3 and data.shape[2] >= 3, "data must be (S, Nsrc, K >= 3), xyz first")
        _require(int(batch_size) >= 1, "batch_size must be positive")
        self.data = data.to(self.device, torch.float32).contiguous()
        if labels.dtype not in _LABEL_DTYPES:
            labels = labels.to(torch.int64)
        self.labels = labels.to(self.device).contiguous()
        S, Nsrc, K = self.data.shape
        self.num_samples = S
        self.batch_size = int(batch_size)
        self.num_points = Nsrc if num_points is None else int(num_points)
        _require(0 <= self.num_points <= Nsrc, "num_points must not exceed the stored clouds'")
        self.num_channels = K
        self.num_batches = S // self.batch_size                                  # the remainder is dropped, :183
        self.training = bool(training)
        augment = self.training and K == 3
        self.rotate = augment if rotate is None else bool(rotate)
        self.jitter = augment if jitter is None else bool(jitter)
        _require(self.training or not (self.rotate or self.jitter), "training=False does not augment")
        self.sort_cloud = bool(sort_cloud)
        self.seed = int(seed)
        self.sigma, self.clip = 0.01, 0.05                                       # jitter_point_cloud's defaults, :64
        per_point = self.labels.dim() == 2
        self._buffers = [BatchBuffers(self.batch_size, self.num_points, K, per_point, self.device, self.sort_cloud,
                                      sort_method=self.sort_method, wide_sort=self.wide_sort) for _ in range(2)]
        self._turn = 0
        self.bad_index = self._buffers[0].bad_index
        self.epoch = -1
        self.next_epoch()

    def _start_epoch(self, epoch, cur_batch):
        self.epoch, self.cur_batch = int(epoch), int(cur_batch)
        if self.training:
            p = np.random.default_rng([self.seed, self.epoch]).permutation(self.num_samples).astype(np.int32)
            self.permutation = torch.from_numpy(p).to(self.device)
        else:
            self.permutation = None

    def next_epoch(self):
        self._start_epoch(self.epoch + 1, 0)

    def has_next_batch(self):
        return self.cur_batch + 1 < self.num_batches

    def next_batch(self):
        self.cur_batch += 1
        return True

    @property
    def step(self):
        return self.epoch * self.num_batches + self.cur_batch

    def get_batch_point_cloud(self, return_randoms=False):
        buf = self._buffers[self._turn]
        if return_randoms and buf.noise is None:
            B, N, K, per_point = buf.shape
            for i in range(2):
                self._buffers[i] = BatchBuffers(B, N, K, per_point, self.device, self.sort_cloud, randoms=True,
                                                sort_method=self.sort_method, wide_sort=self.wide_sort)
            buf = self._buffers[self._turn]
        self._turn ^= 1
        res = assemble_batch(self.data, self.labels, self.batch_size, self.num_points, self.permutation,
                             self.cur_batch * self.batch_size, self.rotate, self.jitter, self.sigma, self.clip,
                             self.sort_cloud, self.seed, self.step, out=buf, return_randoms=return_randoms,
                             sort_method=self.sort_method, wide_sort=self.wide_sort)
        self.bad_index = res[3]
        return res[:3] + res[4:]

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch, "cur_batch": self.cur_batch}

    def load_state_dict(self, state):
        self.seed = int(state["seed"])
        self._start_epoch(state["epoch"], state["cur_batch"])
