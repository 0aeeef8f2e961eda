"""Trainer input paths: the feature-to-feature trainer's files + the pair files of the
feature-to-input / input-to-feature heads (FeatureToInputPreTrainTensorDataset, InputToFeaturePreTrainTensorDataset, PairRing below).

On-disk format (written by DoubleRGBPointFeatures with --save_feature_for_fusion, reference
multiple_features.py:815-825 / 942-945; this package's drop-in writes the same): one ``torch.save``d float32 tensor
``[3136, 1536]`` per sample -- columns 0..767 the Point-MAE patch features, 768..1535 the ViT features resized to
56 x 56 -- under ``<root>/train`` and ``<root>/test``.

* ``PreTrainTensorDataset``  -- the reference's dataset class (dataset.py:247-265): same constructor, ``__len__``,
  ``__getitem__`` -> (tensor on the GPU, 0), same file order (``os.listdir``).
* ``FeatureRing``            -- what replaces ``DataLoader(PreTrainTensorDataset, shuffle=True, num_workers=N,
  multiprocessing_context='forkserver')`` (hallucination_network_pretrain.py:216-225) on the critical path: reader
  threads ``torch.load`` the files of the NEXT batches into pinned staging buffers, a copy stream moves each batch into
  a ring of device-resident ``[B, 3136, 1536]`` buffers, and the training loop receives batches that are already in
  HBM (the reference ``torch.load(..., map_location='cuda')``s inside forked workers, one 19.3 MB file at a time).
  With ``resident=True`` (default when the set fits ``resident_limit_bytes``: the ten MVTec 3D-AD classes are 2 650
  samples x 19.3 MB = 51 GB of the 288 GB HBM) every sample is kept in a device-resident ``[n, 3136, 1536]`` cache the
  first time it is read, and later epochs assemble batches by an on-device gather (616 MB per step at ~5 TB/s) --
  disk and the host are off the critical path from epoch 2 on (a training step is 17.6 ms; torch.load alone sustains
  ~2 GB/s, i.e. 320 ms per batch).
  Batch composition and order are the ones the reference's DataLoader would produce under the same global torch seed
  (RandomSampler draws its permutation seed from the global generator; ``drop_last`` as given), so a run is
  reproducible against the reference sample for sample.

Sample path (second half of this file; docs/sample_prep.md): the reference's ``TrainDataset`` / ``TrainValidationDataset`` /
``TestDataset`` / ``get_data_loader`` over an MVTec 3D-AD directory with a third ``img_process_method``, ``'hip'`` -- files decoded on
reader threads, every transform after that in csrc/sample_prep.hip (``SamplePrep``) -- and ``MVTec3DClass``, the real-data class
source of ``evaluate.evaluate_classes``; ``EyecandiesRawClass`` is the same over the raw Eyecandies download (csrc/eyecandies.hip,
docs/eyecandies.md), ``MVTec3DRawClass`` over the raw MVTec 3D-AD download (csrc/preprocess.hip, docs/preprocessing.md),
``PointCloudClass`` over a tree of unorganised PLY scans (csrc/organize.hip, docs/organize.md; opt-in: ``dataset_classes`` never builds it).
The device sources differ in what they decode and how a batch is prepared, nothing else: ``_device_items`` is their one item
loop (utils.batching.read_ahead decodes ahead, one prepare call per batch, one pinned copy of the masks, batch-of-one items).
"""
import math
import os
import queue
import threading
from pathlib import Path

import torch
from torch.utils.data import Dataset

from .utils.batching import in_batches, read_ahead, scatter_by_shape
from .utils import png
from .utils.png import RawImage
from .utils.tiff import RawCloud


def _shared_stream(device, role):
    from . import ops          # (lazy: this module is importable without the HIP library; the device ring is not usable without it)
    return ops.shared_stream(device, role)


class PreTrainTensorDataset(Dataset):
    def __init__(self, root_path):
        super().__init__()
        self.root_path = root_path
        self.tensor_paths = os.listdir(self.root_path)

    def __len__(self):
        return len(self.tensor_paths)

    def __getitem__(self, idx):
        tensor = torch.load(Path(self.root_path, self.tensor_paths[idx]), map_location="cuda")
        return tensor, 0


# data_type -> ((attribute stem, sub-directory, glob), (…)): the files of a pair, in the reference's attribute names
_PAIR_LAYOUT = {
    "rgb_fxyz": (("rgb", "rgb", "*.pt"), ("fxyz", "fxyz", "*hfxyz.pt")),
    "xyz_frgb": (("frgb", "frgb", "*.pt"), ("xyz", "xyz", "*.pt")),
}


def _discover_pairs(ds, root_path, data_type):
    """Sets <stem>_root_path / <stem>_paths (sorted as plain strings: bagel10 before bagel2, in both lists alike) and `len` on ds,
    the attributes the reference's classes carry; False for a data_type without a layout."""
    layout = _PAIR_LAYOUT.get(data_type)
    if layout is None:
        return False
    counts = []
    for stem, sub, pattern in layout:
        root = Path(root_path, sub)
        paths = sorted(root.glob(pattern))
        setattr(ds, stem + "_root_path", root)
        setattr(ds, stem + "_paths", paths)
        counts.append(len(paths))
    assert counts[0] == counts[1], f"{root_path}: {counts[0]} / {counts[1]} files of the two kinds"
    ds.len = counts[0]
    return True


class FeatureToInputPreTrainTensorDataset(Dataset):
    """The feature-to-INPUT heads' training pairs (reference dataset.py:268-314; selected at
    hallucination_network_pretrain.py:180-201 for RGBFeatureToXYZInput{MLP,Conv} / XYZFeatureToRGBInput{MLP,Conv}).
    Files as DoubleRGBPointFeatures writes them with --save_frgb_xyz / --save_rgb_fxyz (multiple_features.py:827-867, 947-962;
    this package's drop-in writes the same names):
      data_type 'xyz_frgb': <root>/frgb/<class><i>_frgb.pt [3136, 768]  +  <root>/xyz/<class><i>_xyz.pt [3, 224, 224]  -> (frgb, xyz)
      data_type 'rgb_fxyz': <root>/rgb/<class><i>_rgb.pt [3, 224, 224]  +  <root>/fxyz/<class><i>_hfxyz.pt [3136, 768]  -> (fxyz, rgb)
    (the [784, 768] `_lfxyz.pt` files beside them are not read), both loaded straight onto the GPU, the FEATURE first.  Any other
    data_type leaves the object without a length, as the reference does."""

    device = "cuda"      # torch.load(map_location=...) of __getitem__ (the reference hard-codes 'cuda'; CPU tests override it)

    def __init__(self, root_path, data_type):
        super().__init__()
        self.root_path, self.data_type = root_path, data_type
        _discover_pairs(self, root_path, data_type)

    def __len__(self):
        return self.len

    def pair_paths(self, idx):
        """(first, second) file of sample idx, in the order __getitem__ returns them: feature, then input."""
        if self.data_type == "rgb_fxyz":
            return self.fxyz_paths[idx], self.rgb_paths[idx]
        if self.data_type == "xyz_frgb":
            return self.frgb_paths[idx], self.xyz_paths[idx]
        return None

    def __getitem__(self, idx):
        pair = self.pair_paths(idx)
        if pair is None:
            return None          # (the reference's __getitem__ falls through both branches)
        return tuple(torch.load(f, map_location=self.device) for f in pair)


class InputToFeaturePreTrainTensorDataset(Dataset):
    """The input-to-FEATURE (HRNet) heads' training pairs (reference dataset.py:317-362; selected at
    hallucination_network_pretrain.py:203-214 for RGBInputToXYZFeatureHRNET / XYZInputToRGBFeatureHRNET): the same files as
    FeatureToInputPreTrainTensorDataset in the OTHER order -- 'rgb_fxyz' -> (rgb [3,224,224], fxyz [3136,768]),
    'xyz_frgb' -> (xyz, frgb) -- loaded to the HOST (the reference's DataLoader pins and moves them); any other data_type
    raises NotImplementedError."""

    def __init__(self, root_path, data_type):
        super().__init__()
        self.root_path, self.data_type = root_path, data_type
        if not _discover_pairs(self, root_path, data_type):
            raise NotImplementedError

    def __len__(self):
        return self.len

    def pair_paths(self, idx):
        """(first, second) file of sample idx: input, then feature."""
        if self.data_type == "rgb_fxyz":
            return self.rgb_paths[idx], self.fxyz_paths[idx]
        return self.xyz_paths[idx], self.frgb_paths[idx]

    def __getitem__(self, idx):
        return tuple(torch.load(f) for f in self.pair_paths(idx))


class PairRing:
    """What FeatureRing is for the feature-to-feature trainer, for the PAIR datasets above: one epoch of batches
    ``(first [b, ...], second [b, ...])`` already resident in HBM, in the order and composition the reference's
    ``DataLoader(dataset, shuffle=..., batch_size=..., drop_last=...)`` produces under the same global torch seed
    (`epoch_permutation`).  A pair is 9.6 MB + 0.6 MB, the ten MVTec 3D-AD classes 2 650 pairs = 27 GB: every pair is read from disk
    ONCE (the first epoch, `readers` host threads), kept in two device-resident caches, and every later batch is an on-device
    gather -- no DataLoader workers, no per-step H2D.  Works on the host too (device='cpu': tests)."""

    def __init__(self, dataset, batch_size, shuffle=True, drop_last=True, device="cuda", readers=4, rank=0, world=1):
        _check_shard(drop_last, rank, world)
        self.ds, self.batch_size, self.shuffle, self.drop_last = dataset, batch_size, shuffle, drop_last
        self.rank, self.world = rank, world          # data-parallel: this rank's part of every global batch (epoch_batches)
        self.device, self.readers = torch.device(device), readers
        a, b = (torch.load(p, map_location="cpu") for p in dataset.pair_paths(0))
        n = len(dataset)
        self._cache = (torch.empty((n, *a.shape), dtype=a.dtype, device=self.device), torch.empty((n, *b.shape), dtype=b.dtype, device=self.device))
        self._have = torch.zeros(n, dtype=torch.bool)

    def __len__(self):
        return epoch_length(len(self.ds), self.world * self.batch_size, self.drop_last)

    def batches(self):
        return epoch_batches(len(self.ds), self.batch_size, self.shuffle, self.drop_last, self.rank, self.world)

    def _fill(self, idxs):
        todo = [i for i in idxs if not bool(self._have[i])]
        if not todo:
            return

        def one(i):
            pa, pb = self.ds.pair_paths(i)
            return i, torch.load(pa, map_location="cpu"), torch.load(pb, map_location="cpu")

        if self.readers > 1 and len(todo) > 1:
            import concurrent.futures as cf
            with cf.ThreadPoolExecutor(max_workers=self.readers) as ex:
                got = list(ex.map(one, todo))
        else:
            got = [one(i) for i in todo]
        for i, a, b in got:
            self._cache[0][i].copy_(a, non_blocking=True)
            self._cache[1][i].copy_(b, non_blocking=True)
            self._have[i] = True

    def __iter__(self):
        for idxs in self.batches():
            self._fill(idxs)
            sel = torch.tensor(idxs, dtype=torch.int64, device=self.device)
            yield self._cache[0].index_select(0, sel), self._cache[1].index_select(0, sel)


def epoch_permutation(n, shuffle):
    """Index order of one epoch exactly as torch's DataLoader produces it: SequentialSampler, or RandomSampler with
    generator=None (a fresh generator seeded from the GLOBAL generator, then randperm)."""
    torch.empty((), dtype=torch.int64).random_()  # the loader iterator's own base seed, drawn first (torch dataloader.py)
    if not shuffle:
        return list(range(n))
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g).tolist()


def epoch_length(n, batch_size, drop_last):
    """Batches per epoch of n samples: len(DataLoader)."""
    return n // batch_size if drop_last else (n + batch_size - 1) // batch_size


def _check_shard(drop_last, rank, world):
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of world {world}")
    if world > 1 and not drop_last:
        raise ValueError("world > 1 requires drop_last=True: a short last global batch cannot be dealt to the ranks in equal parts")


def epoch_batches(n, batch_size, shuffle, drop_last, rank=0, world=1):
    """One epoch's batches as lists of sample indices: `epoch_permutation` (one call: it consumes the global RNG as the reference's
    DataLoader does) cut into batch_size pieces, a short last one dropped with drop_last.
    world > 1 (data-parallel training, cmdiad_amd/dp_train.py): the same permutation, from the same global-RNG consumption, is cut
    into GLOBAL batches of world * batch_size and rank r gets items [r * batch_size, (r + 1) * batch_size) of each: the ranks
    together see what one process at batch world * batch_size sees, in the same order.  Every rank must be seeded alike (the
    reference's set_seeds(args.seed)); drop_last=True is required."""
    _check_shard(drop_last, rank, world)
    order = epoch_permutation(n, shuffle)
    G = world * batch_size
    return [order[i + rank * batch_size:min(i + G, i + (rank + 1) * batch_size)] for i in range(0, n, G)][:epoch_length(n, G, drop_last)]


class FeatureRing:
    """Iterable over one epoch of batches ``(features [b, rows, cols] on the device, labels [b] zeros)``.

    depth = device buffers in the ring (>= 2: one being consumed, the others filled ahead); a batch stays valid until
    the next one is requested (its refill is ordered after the work the consumer had queued on it).
    readers = host threads decoding files (torch.load releases the GIL while reading)."""

    def __init__(self, root_path, batch_size, shuffle=True, drop_last=True, device="cuda", depth=3, readers=4,
                 resident=True, resident_limit_bytes=200 << 30, rank=0, world=1):
        assert depth >= 2
        _check_shard(drop_last, rank, world)
        self.rank, self.world = rank, world          # data-parallel: this rank's part of every global batch (epoch_batches)
        self.root = root_path
        self.files = os.listdir(root_path)
        self.batch_size, self.shuffle, self.drop_last = batch_size, shuffle, drop_last
        self.device, self.depth, self.readers = torch.device(device), depth, readers
        probe = torch.load(Path(root_path, self.files[0]), map_location="cpu")
        self.sample_shape, self.dtype = tuple(probe.shape), probe.dtype
        pin = self.device.type == "cuda"
        self._staging = [torch.empty((batch_size, *self.sample_shape), dtype=self.dtype, pin_memory=pin) for _ in range(depth)]
        self._dev = [torch.empty((batch_size, *self.sample_shape), dtype=self.dtype, device=self.device) for _ in range(depth)]
        self._copy_stream = _shared_stream(self.device, "dataset.copy") if pin else None
        n_bytes = len(self.files) * probe.numel() * probe.element_size()
        self._cache = None
        self._cached = [False] * len(self.files)
        if resident and pin and n_bytes <= resident_limit_bytes:
            self._cache = torch.empty((len(self.files), *self.sample_shape), dtype=self.dtype, device=self.device)

    def __len__(self):
        return epoch_length(len(self.files), self.world * self.batch_size, self.drop_last)

    def batches(self):
        """The epoch's batches as lists of file indices (consumes the global RNG like the reference's DataLoader)."""
        return epoch_batches(len(self.files), self.batch_size, self.shuffle, self.drop_last, self.rank, self.world)

    def __iter__(self):
        plan = self.batches()
        ready = queue.Queue(maxsize=self.depth - 1)     # filled slots waiting for the consumer
        free = queue.Queue()
        for s in range(self.depth):
            free.put(s)
        stop = threading.Event()

        def load_batch(slot, idxs):
            stage = self._staging[slot]
            if self.readers > 1 and len(idxs) > 1:
                def one(j_i):
                    j, i = j_i
                    stage[j].copy_(torch.load(Path(self.root, self.files[i]), map_location="cpu"))
                threads = [threading.Thread(target=one, args=(ji,)) for ji in enumerate(idxs)]
                live = []
                for t in threads:           # at most `readers` files in flight
                    t.start(); live.append(t)
                    if len(live) >= self.readers:
                        live.pop(0).join()
                for t in live:
                    t.join()
            else:
                for j, i in enumerate(idxs):
                    stage[j].copy_(torch.load(Path(self.root, self.files[i]), map_location="cpu"))

        def producer():
            try:
                for idxs in plan:
                    slot = free.get()
                    if stop.is_set():
                        return
                    ev = None
                    if self._cache is not None and all(self._cached[i] for i in idxs):
                        with torch.cuda.stream(self._copy_stream):  # epoch >= 2: on-device gather, no host work
                            sel = torch.tensor(idxs, dtype=torch.int64).to(self.device, non_blocking=True)
                            torch.index_select(self._cache, 0, sel, out=self._dev[slot][:len(idxs)])
                            ev = torch.cuda.Event()
                            ev.record(self._copy_stream)
                        ready.put((slot, len(idxs), ev))
                        continue
                    load_batch(slot, idxs)
                    if self._copy_stream is not None:
                        with torch.cuda.stream(self._copy_stream):
                            self._dev[slot][:len(idxs)].copy_(self._staging[slot][:len(idxs)], non_blocking=True)
                            if self._cache is not None:
                                sel = torch.tensor(idxs, dtype=torch.int64).to(self.device, non_blocking=True)
                                self._cache.index_copy_(0, sel, self._dev[slot][:len(idxs)])
                                for i in idxs:
                                    self._cached[i] = True
                            ev = torch.cuda.Event()
                            ev.record(self._copy_stream)
                            ev.synchronize()  # the pinned staging buffer of this slot is reused for the next disk batch
                    else:
                        self._dev[slot][:len(idxs)].copy_(self._staging[slot][:len(idxs)])
                    ready.put((slot, len(idxs), ev))
                ready.put(None)
            except BaseException as exc:  # surface reader errors in the training loop, not in a dead thread
                ready.put(exc)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        held = []
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                slot, b, ev = item
                if ev is not None:
                    torch.cuda.current_stream(self.device).wait_event(ev)
                held.append(slot)
                if len(held) > 1:   # the previous batch's buffer may now be refilled
                    done = held.pop(0)
                    if self._copy_stream is not None:  # ... once the consumer's work queued so far has read it
                        ev2 = torch.cuda.Event()
                        ev2.record(torch.cuda.current_stream(self.device))
                        self._copy_stream.wait_event(ev2)
                    free.put(done)
                yield self._dev[slot][:b], torch.zeros(b, dtype=torch.int64)
        finally:
            stop.set()
            for s in range(self.depth):
                free.put(s)
            th.join(timeout=5)


# =========================================================================================== MVTec 3D-AD / Eyecandies samples
# The reference's sample path (dataset.py:12-244, 364-381) and its device form (docs/sample_prep.md).  img_process_method:
#   'cpu_v1'  PIL + torch on the host: the reference's torchvision composition written out (Image.resize(BICUBIC) -> ToTensor ->
#             Normalize; Image.resize(NEAREST) -> ToTensor for the mask) -- the default everywhere, and the yardstick of the device path
#   'cpu_v2'  the reference's torchvision.transforms.v2 spelling of the same pipeline; here an alias of 'cpu_v1'
#   'hip'     decoding on reader threads, everything after it in csrc/sample_prep.hip (SamplePrep); the samples are device tensors
IMG_PROCESS_METHODS = ("cpu_v1", "cpu_v2", "hip")
IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]
DEPTH_SIZE = 224          # dataset.py:109 resizes the depth map without a size: always 224


def eyecandies_classes():
    return ['CandyCane', 'ChocolateCookie', 'ChocolatePraline', 'Confetto', 'GummyBear', 'HazelnutTruffle', 'LicoriceSandwich',
            'Lollipop', 'Marshmallow', 'PeppermintCandy']


def mvtec3d_classes():
    return ["bagel", "cable_gland", "carrot", "cookie", "dowel", "foam", "peach", "potato", "rope", "tire"]


def _check_method(img_process_method):
    if img_process_method not in IMG_PROCESS_METHODS:
        raise ValueError(f"img_process_method must be one of 'cpu_v1', 'cpu_v2', 'hip', got {img_process_method!r}")


# ------------------------------------------------------------------------------------------------ host tables
def _bicubic_filter(x):
    """Pillow's bicubic_filter (a = -0.5), the operations in its order, float64."""
    import numpy as np
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def bicubic_tables(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis of Image.resize(BICUBIC) on 8-bit channels ->
    (coef [n_out, ksize] int32 with 22 fractional bits, bounds [n_out, 2] int32 = (first source index, taps)).  float64, every
    operation in Pillow's order (the weights of a window are summed left to right); docs/sample_prep.md."""
    import numpy as np
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                 # (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    tap = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic_filter(((tap + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where(tap < xmax[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                               # sequential sum, as the C loop (adding 0.0 is exact)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    q = w * float(1 << 22)
    coef = np.where(w < 0, -0.5 + q, 0.5 + q).astype(np.int64).astype(np.int32)     # half away from zero, then (int)
    return coef, np.stack([xmin, xmax], 1).astype(np.int32)


def pillow_nearest_index(n_in, n_out):
    """Source index of every output position under Pillow's Image.resize(NEAREST) (ImagingScaleAffine): the coordinate starts at
    half a step and is ADVANCED by additions in float64, then truncated -- not torch's floor(dst * scale) in float32."""
    import numpy as np
    step = float(n_in) / n_out
    xo = 0.0 + step * 0.5
    out = np.empty(n_out, dtype=np.int32)
    for x in range(n_out):
        out[x] = min(int(xo), n_in - 1)
        xo += step
    return out


def torch_nearest_index(n_in, n_out):
    """torch's mode='nearest' rule (utils.mvtec3d_util._nearest_index) as an int32 table."""
    from .utils.mvtec3d_util import _nearest_index
    return _nearest_index(n_in, n_out).astype("int32")


def normalize_table(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[3,256] float32: ToTensor + Normalize of every uint8 value, computed by torch with torchvision's operations in their order
    (to float32, / 255, - mean, / std) -- the device path looks its floats up here, so it equals the host path by construction."""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).expand(3, 256).clone()
    m = torch.as_tensor(mean, dtype=torch.float32).view(3, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(3, 1)
    return v.sub_(m).div_(s)


# ------------------------------------------------------------------------------------------------ the two host stages, written out
def host_rgb_transform(img, rgb_size):
    """PIL RGB image -> float32 [3,S,S]: transforms.Resize((S,S), BICUBIC) + ToTensor + Normalize (dataset.py:62-65) without torchvision."""
    import numpy as np
    from PIL import Image
    img = img.resize((rgb_size, rgb_size), Image.BICUBIC)
    t = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(IMAGENET_MEAN, dtype=torch.float32).view(3, 1, 1)
    s = torch.as_tensor(IMAGENET_STD, dtype=torch.float32).view(3, 1, 1)
    return t.sub_(m).div_(s)


def host_gt_transform(gt, gt_size):
    """PIL 'L' image -> float32 [1,g,g] in {0, 1}: Resize((g,g), NEAREST) + ToTensor, then > 0.5 (dataset.py:168-171, 239-241)."""
    import numpy as np
    from PIL import Image
    gt = gt.resize((gt_size, gt_size), Image.NEAREST)
    t = torch.from_numpy(np.array(gt, dtype=np.uint8))[None].to(torch.float32).div(255)
    return torch.where(t > 0.5, 1., .0)


def host_cloud_transform(organized_pc, xyz_size):
    """[H,W,3] array -> (resized cloud [3,xs,xs] float32, depth map three times [3,224,224]); dataset.py:108-111."""
    import numpy as np
    from .utils import mvtec3d_util as mu
    depth3 = np.repeat(mu.organized_pc_to_depth_map(organized_pc)[:, :, np.newaxis], 3, axis=2)
    resized_depth = mu.resize_organized_pc(depth3)
    resized_pc = mu.resize_organized_pc(organized_pc, target_height=xyz_size, target_width=xyz_size)
    return resized_pc.clone().detach().float(), resized_depth


# ------------------------------------------------------------------------------------------------ device path
class DeviceSample(tuple):
    """(img, resized_organized_pc, resized_depth_map_3channel) on the device, as the reference's sample tuple, carrying the number of
    valid points of the cloud: ``n_valid_dev`` ([1] int32 on the device) and ``n_valid`` (int; its copy to pinned host memory was
    queued when the sample was prepared -- the first read waits for that copy, nothing else)."""

    def __new__(cls, items, count):
        self = super().__new__(cls, items)
        self._count = count
        return self

    @property
    def n_valid_dev(self):
        return self._count.dev()

    @property
    def n_valid(self):
        return self._count.host()

    def batched(self):
        """The same sample as a DataLoader with batch_size=1 hands it out: every tensor with a leading 1."""
        return DeviceSample(tuple(t.unsqueeze(0) for t in self), self._count)


class _Count:
    def __init__(self, dev, host, event, i):
        self._dev, self._host, self._event, self._i, self._value = dev, host, event, i, None

    def dev(self):
        return self._dev[self._i:self._i + 1]

    def host(self):
        if self._value is None:
            self._event.synchronize()
            self._value = int(self._host[self._i])
        return self._value


def _is_raw(cloud):
    """A utils.tiff.RawCloud (the bytes of an xyz tiff, CMDIAD_TIFF_DEVICE=1) in the place of a decoded cloud array."""
    return isinstance(cloud, RawCloud)


def _is_raw_image(img):
    """A utils.png.RawImage (the filtered scanlines of a PNG, CMDIAD_PNG_DEVICE=1) in the place of a decoded rgb or gt array."""
    return isinstance(img, RawImage)


def _shape(a):
    """The shape of a decoded array, or of the array a RawCloud / RawImage stands for."""
    import numpy as np
    return tuple(a.shape) if _is_raw(a) or _is_raw_image(a) else np.shape(a)


class SamplePrep:
    """Decoded arrays -> the tensors of the reference's ``__getitem__`` on the device (csrc/sample_prep.hip; docs/sample_prep.md).

    ``prepare(rgb_u8 [H,W,3], pc [H,W,3] float32 or float64, gt_u8 [H,W] | None)`` -> ``(DeviceSample(img [3,S,S], cloud [3,xs,xs], depth [3,224,224]),
    gt [1,g,g] | None)``; ``prepare_batch`` takes lists and returns a list of such pairs.  A cloud may also be a utils.tiff.RawCloud -- the
    undecoded bytes of its tiff (CMDIAD_TIFF_DEVICE=1) -- which is unpacked on the device and gives the same tensors; an rgb or a gt may be a
    utils.png.RawImage -- the filtered scanlines of its PNG (CMDIAD_PNG_DEVICE=1) -- whose filters are undone on the device.  Samples of equal shapes share their launches;
    every sample's bytes are the ones a call of its own gives (the arithmetic is per pixel and integer).  Clouds are grouped by dtype
    as well: a float64 cloud (an Eyecandies tiff of the reference's script) is converted to float32 at the gather, as ``.float()``.  Inputs go up through
    pinned memory on the shared copy stream; the kernels run on the current stream.  Tables are computed once per (n_in, n_out)
    and kept on the device."""

    def __init__(self, rgb_size=224, xyz_size=224, gt_size=224, device="cuda"):
        self.rgb_size, self.xyz_size, self.gt_size = int(rgb_size), int(xyz_size), int(gt_size)
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            from . import _native as nat
            raise nat.NativeError("SamplePrep needs a GPU: img_process_method='hip' has no CPU path (use 'cpu_v1' on the host)")
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        self._tables = {}
        self._copy_stream = _shared_stream(self.device, "dataset.copy")

    def _table(self, kind, n_in, n_out):
        key = (kind, n_in, n_out)
        t = self._tables.get(key)
        if t is None:
            if kind == "bicubic":
                t = tuple(torch.from_numpy(a).to(self.device) for a in bicubic_tables(n_in, n_out))
            elif kind == "norm":
                t = normalize_table().to(self.device)
            else:
                fn = pillow_nearest_index if kind == "pillow" else torch_nearest_index
                t = torch.from_numpy(fn(n_in, n_out)).to(self.device)
            self._tables[key] = t
        return t

    def _upload(self, arrays, dtype, what):
        """list of equal-shaped numpy arrays -> one device tensor [n, ...], through pinned memory on the copy stream."""
        import numpy as np
        first = np.asarray(arrays[0])
        host = torch.empty((len(arrays), *first.shape), dtype=dtype, pin_memory=True)
        view = host.numpy()
        for i, a in enumerate(arrays):
            a = np.asarray(a)
            if a.dtype != view.dtype or a.shape != first.shape:
                raise TypeError(f"SamplePrep: {what} must be {view.dtype} arrays of one shape per group, got {a.dtype} {a.shape}")
            view[i] = a
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._copy_stream):
            dev = host.to(self.device, non_blocking=True)
        cur.wait_stream(self._copy_stream)
        dev.record_stream(cur)
        return dev

    def _merged(self, n, parts, dtype):
        """parts = ((rows, tensor [len(rows), ...]), ...) covering 0..n-1 -> one tensor [n, ...] with every part at its rows."""
        out = torch.empty((n, *parts[0][1].shape[1:]), dtype=dtype, device=self.device)
        for rows, part in parts:      # (a pinned index: the copy of a pageable one would synchronise)
            out.index_copy_(0, torch.tensor(rows, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True), part)
        return out

    def _upload_images(self, images, what):
        """list of equal-shaped uint8 images, decoded arrays or utils.png.RawImage -> one device tensor [n, ...]: the arrays through
        `_upload`, the raw files through png.decode_on_device (their scanlines go up filtered and cmdiad_png_unfilter undoes them)."""
        raw = [k for k, a in enumerate(images) if _is_raw_image(a)]
        if not raw:
            return self._upload(images, torch.uint8, what)
        dev = png.decode_on_device([images[k] for k in raw], self.device)
        if len(raw) == len(images):
            return dev
        is_raw = set(raw)
        host = [k for k in range(len(images)) if k not in is_raw]
        up = self._upload([images[k] for k in host], torch.uint8, what)
        if up.shape[1:] != dev.shape[1:]:
            raise TypeError(f"SamplePrep: {what} must be arrays of one shape per group, got {tuple(up.shape[1:])} beside {tuple(dev.shape[1:])}")
        return self._merged(len(images), ((raw, dev), (host, up)), torch.uint8)

    def _upload_clouds(self, clouds, dtype):
        """list of equal-shaped clouds, decoded arrays or utils.tiff.RawCloud -> one device tensor [n,H,W,3] of dtype: the arrays through
        `_upload`, the raw files through tiff.unpack_on_device (their bytes go up as they are and are unpacked by cmdiad_tiff_unpack)."""
        raw = [k for k, c in enumerate(clouds) if _is_raw(c)]
        if not raw:
            return self._upload(clouds, dtype, "the point cloud")
        from .utils import tiff
        for k in raw:
            if getattr(torch, clouds[k].dtype.name) != dtype:
                raise TypeError(f"SamplePrep: the point cloud must be {dtype} in this group, got {clouds[k].dtype} ({clouds[k].path})")
        dev = tiff.unpack_on_device([clouds[k] for k in raw], self.device)
        if len(raw) == len(clouds):
            return dev
        is_raw = set(raw)
        host = [k for k in range(len(clouds)) if k not in is_raw]
        up = self._upload([clouds[k] for k in host], dtype, "the point cloud")
        return self._merged(len(clouds), ((raw, dev), (host, up)), dtype)

    def prepare(self, rgb_u8, pc_f32, gt_u8=None):
        return self.prepare_batch([rgb_u8], [pc_f32], [gt_u8])[0]

    def prepare_batch(self, rgbs, pcs, gts=None):
        import numpy as np
        from . import ops
        n = len(rgbs)
        gts = list(gts) if gts is not None else [None] * n
        if not (len(pcs) == len(gts) == n):
            raise ValueError("SamplePrep.prepare_batch: the lists differ in length")
        for r, p, g in zip(rgbs, pcs, gts):
            rs, ps, gs = _shape(r), _shape(p), (None if g is None else _shape(g))
            if len(rs) != 3 or rs[2] != 3 or len(ps) != 3 or ps[2] != 3 or (gs is not None and len(gs) != 2):
                raise ValueError(f"SamplePrep: rgb [H,W,3], cloud [H,W,3], gt [H,W] expected, got {rs}, {tuple(ps)}, {gs}")

        def clouds_of(key, idx):
            dtype = key[1]
            if dtype not in ("float32", "float64"):
                raise TypeError(f"SamplePrep: the point cloud must be float32 (MVTec 3D-AD) or float64 (Eyecandies) arrays, got {dtype}")
            return self.prepare_device_clouds(self._upload_clouds([pcs[i] for i in idx], getattr(torch, dtype)))

        with torch.cuda.device(self.device):
            imgs = self.prepare_images(rgbs)
            clouds = scatter_by_shape(pcs, range(n), clouds_of, with_dtype=True)
            masks = self.prepare_masks(gts)
        return [(DeviceSample((imgs[i], *clouds[i][:2]), clouds[i][2]), masks[i]) for i in range(n)]

    def prepare_images(self, rgbs):
        """list of uint8 [H,W,3] arrays (or utils.png.RawImage of target 'rgb') -> list of float32 [3,S,S] device tensors (resize +
        ToTensor + Normalize)."""
        with torch.cuda.device(self.device):
            return scatter_by_shape(rgbs, range(len(rgbs)),
                                    lambda _, idx: self.prepare_device_images(self._upload_images([rgbs[i] for i in idx], "rgb")))

    def prepare_device_images(self, src):
        """src [B,H,W,3] uint8 ON THE DEVICE -> float32 [B,3,S,S] on the current stream (resize + ToTensor + Normalize)."""
        from . import ops
        if src.dim() != 4:
            raise ValueError(f"SamplePrep: rgb must be [B,H,W,3], got {tuple(src.shape)}")
        _, H, W, _ = src.shape
        S = self.rgb_size
        with torch.cuda.device(self.device):
            htab = self._table("bicubic", W, S) if W != S else None
            vtab = self._table("bicubic", H, S) if H != S else None
            return ops.resize_bicubic_u8(src, S, S, htab, vtab, self._table("norm", 256, 3))[1]

    def prepare_device_clouds(self, src):
        """src [B,H,W,3] float32 or float64 ON THE DEVICE -> list of (cloud [3,xs,xs], depth [3,224,224], _Count) per sample, on the
        current stream; the counts' copy to pinned host memory is queued behind the kernels."""
        from . import ops
        B, H, W, _ = src.shape
        with torch.cuda.device(self.device):
            cloud, depth, count = ops.organized_pc_prep(
                src, (self._table("torch", H, self.xyz_size), self._table("torch", W, self.xyz_size)),
                (self._table("torch", H, DEPTH_SIZE), self._table("torch", W, DEPTH_SIZE)))
            host = torch.empty(B, dtype=torch.int32, pin_memory=True)
            host.copy_(count, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        return [(cloud[j], depth[j], _Count(count, host, event, j)) for j in range(B)]

    def prepare_masks(self, gts):
        """list of uint8 [H,W] arrays (or utils.png.RawImage of target 'l') or None -> list of float32 [1,g,g] device tensors or None."""
        with torch.cuda.device(self.device):
            return scatter_by_shape(gts, [i for i in range(len(gts)) if gts[i] is not None],
                                    lambda _, idx: self.prepare_device_masks(self._upload_images([gts[i] for i in idx], "gt")))

    def prepare_device_masks(self, src):
        """src [B,H,W] uint8 ON THE DEVICE -> float32 [B,1,g,g] in {0, 1} on the current stream (Pillow's NEAREST resize, ToTensor, > 0.5)."""
        from . import ops
        if src.dim() != 3:
            raise ValueError(f"SamplePrep: gt must be [B,H,W], got {tuple(src.shape)}")
        _, H, W = src.shape
        with torch.cuda.device(self.device):
            return ops.gt_mask_prep(src, (self._table("pillow", H, self.gt_size), self._table("pillow", W, self.gt_size)))


class _LazySamplePrep:
    """``sample_prep()``: the SamplePrep of the object's rgb_size / xyz_size / gt_size, built at first use (it needs a GPU; ``_prep`` is
    None until then)."""
    _prep = None

    def sample_prep(self):
        if self._prep is None:
            self._prep = SamplePrep(self.rgb_size, self.xyz_size, self.gt_size)
        return self._prep


# ------------------------------------------------------------------------------------------------ the reference's dataset classes
def _sorted_glob(*parts):
    pattern = parts[-1]
    paths = list(Path(*parts[:-1]).glob(pattern))
    paths.sort()
    return paths


def _read_rgb(path):
    from PIL import Image
    return Image.open(path).convert('RGB')


def _raw_png(path, target, color_types=(0, 2, 4, 6)):
    """Under CMDIAD_PNG_DEVICE=1 (read here, per file, on a 'hip' reader thread): the utils.png.RawImage of a PNG the device decodes
    -- its scanlines inflated here, their filters undone on the device with the batch (docs/png.md) -- else None: the caller decodes
    the file with Pillow as before (switch off, or a file outside the subset: palette, 16-bit, interlaced, ...)."""
    if not png.device_decode_enabled():
        return None
    return png.read_for_device(path, target, color_types)


def _read_cloud(path, raw_ok=False):
    """The cloud of an xyz tiff: the decoded array, or -- raw_ok (a 'hip' reader thread) under CMDIAD_TIFF_DEVICE=1 -- the file's bytes
    as a utils.tiff.RawCloud, unpacked on the device with its batch (docs/tiff.md)."""
    if raw_ok:
        from .utils import tiff
        if tiff.device_decode_enabled():
            return tiff.read_raw(path)
    from .utils import mvtec3d_util as mu
    return mu.read_tiff_organized_pc(path)     # (looked up at call time: `tifffile` when it is installed, else utils/tiff.py)


class BaseAnomalyDetectionDataset(_LazySamplePrep, Dataset):
    """dataset.py:45-70.  `decoded(idx)` returns what the files hold (the part that stays on the host whatever the method);
    `__getitem__` the reference's item: with 'cpu_v1' / 'cpu_v2' host tensors, with 'hip' device tensors (one SamplePrep call per
    item; `get_data_loader` batches the calls)."""

    def __init__(self, split, class_name, rgb_size, xyz_size, gt_size, dataset_path, img_process_method):
        _check_method(img_process_method)
        self.IMAGENET_MEAN, self.IMAGENET_STD = list(IMAGENET_MEAN), list(IMAGENET_STD)
        self.cls, self.rgb_size, self.xyz_size, self.gt_size = class_name, rgb_size, xyz_size, gt_size
        if split == 'train_validation':
            self.img_path = str(Path(dataset_path, self.cls, 'train'))
            self.img_path2 = str(Path(dataset_path, self.cls, 'validation'))
        else:
            self.img_path = str(Path(dataset_path, self.cls, split))
        self.img_process_method = img_process_method

    def __len__(self):
        return len(self.img_paths)

    def decoded(self, idx):
        """(rgb uint8 [H,W,3], cloud [H,W,3], gt uint8 [H,W] or None) of item idx: the decoded files, nothing else.  Under 'hip' the
        cloud may be a RawCloud (CMDIAD_TIFF_DEVICE=1), the rgb and the gt a RawImage (CMDIAD_PNG_DEVICE=1)."""
        import numpy as np
        rgb_path, tiff_path = self.img_paths[idx]
        hip = self.img_process_method == 'hip'
        gt = getattr(self, "gt_paths", None)
        gt = gt[idx] if gt is not None else 0
        if gt != 0:
            gt_path, gt = gt, None
            if hip:
                gt = _raw_png(gt_path, 'l')
            if gt is None:
                from PIL import Image
                gt = np.array(Image.open(gt_path).convert('L'), dtype=np.uint8)
        cloud = _read_cloud(tiff_path, raw_ok=hip)
        rgb = _raw_png(rgb_path, 'rgb') if hip else None
        if rgb is None:
            rgb = np.array(_read_rgb(rgb_path), dtype=np.uint8)
        return rgb, cloud, (None if isinstance(gt, int) else gt)

    def _sample(self, idx):
        rgb_path, tiff_path = self.img_paths[idx]
        if self.img_process_method == 'hip':
            rgb, pc, _ = self.decoded(idx)
            return self.sample_prep().prepare(rgb, pc)[0]
        img = host_rgb_transform(_read_rgb(rgb_path), self.rgb_size)
        resized_pc, resized_depth = host_cloud_transform(_read_cloud(tiff_path), self.xyz_size)
        return img, resized_pc, resized_depth

    def _good_pairs(self, *roots):
        rgb_paths, tiff_paths = [], []
        for root in roots:
            rgb_paths += list(Path(root, 'good', 'rgb').glob("*.png"))
            tiff_paths += list(Path(root, 'good', 'xyz').glob("*.tiff"))
        rgb_paths.sort()
        tiff_paths.sort()
        return list(zip(rgb_paths, tiff_paths))


class TrainDataset(BaseAnomalyDetectionDataset):
    """dataset.py:73-113: good/rgb/*.png zipped with good/xyz/*.tiff, both sorted; label 0."""

    def __init__(self, class_name, rgb_size, xyz_size, gt_size, dataset_path, img_process_method):
        super().__init__(split="train", class_name=class_name, rgb_size=rgb_size, xyz_size=xyz_size, gt_size=gt_size,
                         dataset_path=dataset_path, img_process_method=img_process_method)
        self.img_paths, self.labels = self.load_dataset()  # self.labels => good : 0, anomaly : 1

    def load_dataset(self):
        pairs = self._good_pairs(self.img_path)
        return pairs, [0] * len(pairs)

    def __getitem__(self, idx):
        return self._sample(idx), self.labels[idx]


class TrainValidationDataset(TrainDataset):
    """dataset.py:116-160: the good samples of train/ and validation/ together, sorted as one list."""

    def __init__(self, class_name, rgb_size, xyz_size, gt_size, dataset_path, img_process_method):
        BaseAnomalyDetectionDataset.__init__(self, split="train_validation", class_name=class_name, rgb_size=rgb_size, xyz_size=xyz_size,
                                             gt_size=gt_size, dataset_path=dataset_path, img_process_method=img_process_method)
        self.img_paths, self.labels = self.load_dataset()

    def load_dataset(self):
        pairs = self._good_pairs(self.img_path, self.img_path2)
        return pairs, [0] * len(pairs)


class TestDataset(BaseAnomalyDetectionDataset):
    """dataset.py:163-244.  The defect directories are visited in SORTED order: the reference walks os.listdir(), whose order is
    unspecified; sorted is one of the orders it can produce (and the one that makes a run reproducible across file systems)."""
    __test__ = False      # (not a pytest class)

    def __init__(self, class_name, rgb_size, xyz_size, gt_size, dataset_path, img_process_method):
        super().__init__(split="test", class_name=class_name, rgb_size=rgb_size, xyz_size=xyz_size, gt_size=gt_size,
                         dataset_path=dataset_path, img_process_method=img_process_method)
        self.img_paths, self.gt_paths, self.labels = self.load_dataset()  # self.labels => good : 0, anomaly : 1

    def load_dataset(self):
        img_tot_paths, gt_tot_paths, tot_labels = [], [], []
        for defect_type in sorted(os.listdir(self.img_path)):
            rgb_paths = _sorted_glob(self.img_path, defect_type, 'rgb', "*.png")
            tiff_paths = _sorted_glob(self.img_path, defect_type, 'xyz', "*.tiff")
            sample_paths = list(zip(rgb_paths, tiff_paths))
            img_tot_paths.extend(sample_paths)
            if defect_type == 'good':
                gt_tot_paths.extend([0] * len(sample_paths))
                tot_labels.extend([0] * len(sample_paths))
            else:
                gt_tot_paths.extend(_sorted_glob(self.img_path, defect_type, 'gt', "*.png"))
                tot_labels.extend([1] * len(sample_paths))
        assert len(img_tot_paths) == len(gt_tot_paths), "Something wrong with test and ground truth pair!"
        return img_tot_paths, gt_tot_paths, tot_labels

    def __getitem__(self, idx):
        gt, label = self.gt_paths[idx], self.labels[idx]
        rgb_path = str(self.img_paths[idx][0])
        if self.img_process_method == 'hip':
            rgb, pc, gt_u8 = self.decoded(idx)
            sample, gt = self.sample_prep().prepare(rgb, pc, gt_u8)
            if gt is None:
                gt = torch.zeros([1, DEPTH_SIZE, DEPTH_SIZE], device=sample[0].device)
            return sample, gt[:1], label, rgb_path
        sample = self._sample(idx)
        if gt == 0:
            gt = torch.zeros([1, sample[2].size()[-2], sample[2].size()[-2]])
        else:
            from PIL import Image
            gt = host_gt_transform(Image.open(gt).convert('L'), self.gt_size)
        return sample, gt[:1], label, rgb_path     # only need 1 dimension gt instead of 3


class DeviceSampleLoader:
    """What ``DataLoader(dataset, batch_size=1, shuffle=False, num_workers=6, prefetch_factor=6, pin_memory=True)`` (dataset.py:377)
    is for img_process_method='hip': the same items in the same order -- ``((img, cloud, depth), label)`` or ``((img, cloud, depth), gt,
    label, [rgb_path])``, every tensor with the leading 1 of a batch of one -- with the sample tensors ON THE DEVICE (a DeviceSample:
    the valid-point count rides along).  ``readers`` host threads decode the PNG / tiff files of the next samples; this thread hands
    ``batch`` decoded samples at a time to SamplePrep.  Threads, not worker processes: a child process that has not initialised the
    GPU must not be handed device state.  The mask is yielded on the HOST (one pinned copy per batch): its only consumers are the
    metric lists."""

    def __init__(self, dataset, readers=6, batch=16, prep=None):
        self.dataset, self.readers, self.batch = dataset, max(1, int(readers)), max(1, int(batch))
        self.prep = prep if prep is not None else dataset.sample_prep()

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        ds = self.dataset
        return _device_items(len(ds), ds.decoded, lambda dec: self.prep.prepare_batch(*zip(*dec)), ds.labels,
                             [str(p[0]) for p in ds.img_paths] if hasattr(ds, "gt_paths") else None, self.readers, self.batch)


def _device_items(n, decode, prepare, labels, rgb_paths, readers, batch):
    """The item stream of every device source, in index order: ``(sample.batched(), label [1])`` or, with ``rgb_paths`` (a test split),
    ``(sample.batched(), host mask [1,1,g,g], label [1], [rgb_path])``.  ``decode(i)`` runs on ``readers`` threads, up to
    ``max(2 * readers, batch)`` items ahead; ``prepare(list of decoded) -> [(DeviceSample, mask | None)]`` runs here, once per ``batch``
    items, and the batch's masks go to the host through one pinned copy.  A decode error surfaces when its batch is gathered: the
    batches before it have been yielded.  The reader pool belongs to the `read_ahead` generator: when ``prepare`` or the consumer
    fails, it is shut down by that generator's close as this one is finalised."""
    lo = 0
    for dec in in_batches(read_ahead(decode, range(n), readers, max(2 * readers, batch)), batch):
        out = prepare(dec)
        masks = _masks_to_host([m for _, m in out]) if rgb_paths is not None else None
        for j, (sample, _) in enumerate(out):
            label = torch.tensor([labels[lo + j]])
            if rgb_paths is not None:
                yield sample.batched(), masks[j], label, [rgb_paths[lo + j]]
            else:
                yield sample.batched(), label
        lo += len(dec)
        del dec      # a batch's decoded arrays (150 MB at 800 x 800) go before the next are taken: the readers' allocations reuse them


def _masks_to_host(masks):
    """device masks [1,g,g] (None: a good sample) -> host masks [1,1,g,g], through one pinned copy."""
    have = [m for m in masks if m is not None]
    host = None
    if have:
        host = torch.empty((len(have), *have[0].shape), dtype=torch.float32, pin_memory=True)
        host.copy_(torch.stack(have), non_blocking=True)
        torch.cuda.current_stream(have[0].device).synchronize()
    out, k = [], 0
    for m in masks:
        if m is None:
            out.append(torch.zeros([1, 1, DEPTH_SIZE, DEPTH_SIZE]))
        else:
            out.append(host[k][None].clone())
            k += 1
    return out


def get_data_loader(split, class_name, rgb_size, xyz_size, gt_size, args):
    """dataset.py:364-381.  args.dataset_path, args.img_process_method (default 'cpu_v1'); args.num_workers (default 6: the reference's
    worker processes for the host methods, the reader THREADS of 'hip')."""
    classes = {'train': TrainDataset, 'train_validation': TrainValidationDataset, 'test': TestDataset}
    if split not in classes:
        raise ValueError
    method = getattr(args, "img_process_method", "cpu_v1")
    dataset = classes[split](class_name=class_name, rgb_size=rgb_size, xyz_size=xyz_size, gt_size=gt_size,
                             dataset_path=args.dataset_path, img_process_method=method)
    workers = int(getattr(args, "num_workers", 6))
    if method == 'hip':
        return DeviceSampleLoader(dataset, readers=workers)
    from torch.utils.data import DataLoader
    return DataLoader(dataset=dataset, batch_size=1, shuffle=False, num_workers=workers, drop_last=False,
                      prefetch_factor=6 if workers > 0 else None, pin_memory=torch.cuda.is_available())


class MVTec3DClass:
    """One class directory of MVTec 3D-AD (or of an Eyecandies tree preprocessed by the reference's script: the same layout) as the
    data object of evaluate.ClassRun / evaluate_classes: ``name``, ``n_train``, ``n_test``, ``train()`` yielding ``(sample, label)`` and
    ``test()`` yielding ``(sample, mask, label, rgb_path)`` -- the reference's two loaders (cmdiad_runner.py:36-42, 77-78), with
    ``args.img_process_method`` choosing the host or the device path and ``args.train_with_validation`` the train split."""

    def __init__(self, dataset_path, class_name, args):
        import types
        self.name = class_name
        self.args = types.SimpleNamespace(**{**vars(args), "dataset_path": dataset_path})
        a = self.args
        self._sizes = dict(rgb_size=getattr(a, "rgb_size", 224), xyz_size=getattr(a, "xyz_size", 224), gt_size=getattr(a, "gt_size", 224))
        self._train_split = "train_validation" if getattr(a, "train_with_validation", False) else "train"
        self.n_train = len(self._loader(self._train_split).dataset)
        self.n_test = len(self._loader("test").dataset)

    def _loader(self, split):
        return get_data_loader(split, class_name=self.name, args=self.args, **self._sizes)

    def train(self):
        return iter(self._loader(self._train_split))

    def test(self):
        return iter(self._loader("test"))


class _RawClassSource(_LazySamplePrep):
    """What the two raw-download class sources share: 'hip' or an error, the three sizes of ``args``, ``readers`` (args.num_workers) and
    ``batch``, the SamplePrep built at first use, and `_device_items` over the subclass's ``_prepare``.  A subclass sets
    ``_no_host_path``, its whole error text with a ``{method!r}`` field."""

    def __init__(self, class_name, args):
        method = getattr(args, "img_process_method", "cpu_v1")
        _check_method(method)
        if method != 'hip':
            raise ValueError(self._no_host_path.format(method=method))
        self.name, self.args = class_name, args
        self.rgb_size, self.xyz_size, self.gt_size = (getattr(args, k, 224) for k in ("rgb_size", "xyz_size", "gt_size"))
        self.readers, self.batch = max(1, int(getattr(args, "num_workers", 6))), 16

    def _items(self, n, decode, labels, rgb_paths=None):
        return _device_items(n, decode, self._prepare, labels, rgb_paths, self.readers, self.batch)


class EyecandiesRawClass(_RawClassSource):
    """One class directory of the RAW Eyecandies download (``<class>/train/data/{i:03d}_*``, ``<class>/test_public/data/{i:02d}_*``) as the
    data object of evaluate.ClassRun / evaluate_classes, with MVTec3DClass's protocol.  It yields what MVTec3DClass with
    img_process_method='hip' yields over the tree the reference's utils/preprocessing_eyecandies.py would have written from this
    directory, without that tree: reader threads decode the 16-bit depth PNG, the yaml, the pose and the images; every batch is one
    ``eyecandies_cloud`` -> ``organized_pc_prep`` chain on the current stream, and the float64 cloud never leaves the device
    (docs/eyecandies.md).  Test order: the `bad` samples in index order, then the `good` ones (TestDataset's sorted directories);
    label 1 / 0; a good sample's mask is zeros; ``rgb_path`` is the raw ``*_image_4.png``.  There is no host path."""
    _no_host_path = ("EyecandiesRawClass: the raw Eyecandies download is prepared on the device only, there is no host path: "
                     "img_process_method must be 'hip', got {method!r} (or run utils/preprocessing_eyecandies.py first and "
                     "point dataset_path at its tree)")

    def __init__(self, dataset_path, class_name, args):
        from .utils import preprocessing_eyecandies as pe
        super().__init__(class_name, args)
        self.focal_length = pe.FOCAL_LENGTH
        self._train_dir = str(Path(dataset_path, class_name, "train", "data"))
        self._test_dir = str(Path(dataset_path, class_name, "test_public", "data"))
        self.n_train = pe.raw_samples(self._train_dir, 3)
        self.n_test = pe.raw_samples(self._test_dir, 2)
        self._train_files = [pe.sample_files(self._train_dir, i, 3) for i in range(self.n_train)]
        test_files = [pe.sample_files(self._test_dir, i, 2) for i in range(self.n_test)]
        import numpy as np
        is_bad = [bool(np.any(pe.read_mask(f["mask"]))) for f in test_files]
        order = [i for i in range(self.n_test) if is_bad[i]] + [i for i in range(self.n_test) if not is_bad[i]]
        self.test_indices = order                                  # raw index of every test item
        self.test_labels = [1 if is_bad[i] else 0 for i in order]
        self._test_files = [test_files[i] for i in order]

    def _decode(self, files, label):
        import numpy as np
        from .utils import preprocessing_eyecandies as pe
        gt = None
        if label:
            gt = _raw_png(files["mask"], 'l')        # (.convert('RGB').convert('L') equals .convert('L') for the types the device decodes)
            if gt is None:
                from PIL import Image
                gt = np.array(Image.open(files["mask"]).convert('RGB').convert('L'), dtype=np.uint8)
        rgb = _raw_png(files["rgb"], 'rgb')
        if rgb is None:
            rgb = np.array(_read_rgb(files["rgb"]), dtype=np.uint8)
        return rgb, pe.read_scan(files["depth"], files["info"], files["pose"]), gt

    def _prepare(self, dec):
        """decoded samples -> [(DeviceSample, mask or None)]: per shape one upload of the codes and one kernel chain."""
        from .utils import preprocessing_eyecandies as pe
        prep = self.sample_prep()
        imgs = prep.prepare_images([d[0] for d in dec])
        masks = prep.prepare_masks([d[2] for d in dec])

        def clouds_of(_, idx):
            codes, minds, maxds, poses = zip(*(dec[i][1] for i in idx))
            cloud, _ = pe.cloud_on_device(codes, minds, maxds, poses, self.focal_length, prep.device, want_removed=False)
            return prep.prepare_device_clouds(cloud)

        with torch.cuda.device(prep.device):
            clouds = scatter_by_shape([d[1][0] for d in dec], range(len(dec)), clouds_of)
        return [(DeviceSample((img, cloud, depth), count), mask) for img, (cloud, depth, count), mask in zip(imgs, clouds, masks)]

    def train(self):
        files = self._train_files
        return self._items(self.n_train, lambda i: self._decode(files[i], 0), [0] * self.n_train)

    def test(self):
        files, labels = self._test_files, self.test_labels
        return self._items(self.n_test, lambda i: self._decode(files[i], labels[i]), labels, [f["rgb"] for f in files])


class MVTec3DRawClass(_RawClassSource):
    """One class directory of the RAW MVTec 3D-AD download -- the tree on which the reference's utils/preprocessing.py has NOT been
    run -- as the data object of evaluate.ClassRun / evaluate_classes, with MVTec3DClass's protocol.  It yields, sample for sample and
    bit for bit, what MVTec3DClass with img_process_method='hip' yields over a copy of the tree that utils.preprocessing.
    preprocess_dataset has cleaned, without writing anything: reader threads decode rgb, tiff and gt as the script decodes them,
    every batch goes up through pinned memory on the shared copy stream, every scan runs ``preprocess_on_device`` (plane removal,
    padding, largest DBSCAN cluster; docs/preprocessing.md) and SamplePrep's device entry points.  Files, order, labels and
    ``rgb_path`` are TrainDataset's / TrainValidationDataset's / TestDataset's; a good test sample's mask is zeros.  There is no host
    path."""
    _no_host_path = ("MVTec3DRawClass: raw MVTec 3D-AD scans are cleaned on the device only, there is no host path: "
                     "img_process_method must be 'hip', got {method!r} (or run utils/preprocessing.py over the tree first and "
                     "read it with MVTec3DClass: raw_scans=False)")

    def __init__(self, dataset_path, class_name, args):
        super().__init__(class_name, args)
        sizes = dict(class_name=class_name, rgb_size=self.rgb_size, xyz_size=self.xyz_size, gt_size=self.gt_size,
                     dataset_path=dataset_path, img_process_method='hip')
        self._train = (TrainValidationDataset if getattr(args, "train_with_validation", False) else TrainDataset)(**sizes)
        self._test = TestDataset(**sizes)
        self.n_train, self.n_test = len(self._train), len(self._test)

    @staticmethod
    def _decode(paths, gt_path):
        """(cloud, rgb, gt or None) as utils.preprocessing._read decodes them: the arrays the files hold, unconverted."""
        import numpy as np
        from PIL import Image
        rgb_path, tiff_path = paths
        pc = _read_cloud(tiff_path, raw_ok=True)
        pc = pc if _is_raw(pc) else np.asarray(pc)     # (a RawCloud carries the layout's dtype and shape: the checks below read those)
        rgb = _raw_png(rgb_path, 'raw', color_types=(2,))       # (any other file: Pillow, and the checks below)
        if rgb is None:
            rgb = np.array(Image.open(rgb_path))
        gt = _raw_png(gt_path, 'raw', color_types=(0,)) if gt_path is not None else None
        if gt is None and gt_path is not None:
            gt = np.array(Image.open(gt_path))
        if pc.dtype != np.float32 or pc.ndim != 3 or pc.shape[2] != 3:
            raise TypeError(f"MVTec3DRawClass: {tiff_path}: the point cloud must be a float32 [H,W,3] array, got {pc.dtype} {pc.shape}")
        if rgb.dtype != np.uint8 or rgb.shape != tuple(pc.shape):
            raise TypeError(f"MVTec3DRawClass: {rgb_path}: rgb must be a uint8 {pc.shape} array, got {rgb.dtype} {rgb.shape}")
        if gt is not None and (gt.dtype != np.uint8 or gt.shape != pc.shape[:2]):
            raise TypeError(f"MVTec3DRawClass: {gt_path}: gt must be a uint8 {pc.shape[:2]} array, got {gt.dtype} {gt.shape}")
        return pc, rgb, gt

    def _prepare(self, dec):
        """decoded scans -> [(DeviceSample, mask or None)]: one upload per shape, one cleaning chain and one preparation per scan."""
        from .utils import preprocessing as pp
        prep = self.sample_prep()

        def scans_of(_, idx):
            pcs = prep._upload_clouds([dec[i][0] for i in idx], torch.float32)
            rgbs = prep._upload_images([dec[i][1] for i in idx], "rgb")
            with_gt = [i for i in idx if dec[i][2] is not None]
            gts = prep._upload_images([dec[i][2] for i in with_gt], "gt") if with_gt else None
            gt_row = {i: k for k, i in enumerate(with_gt)}
            out = []
            for j, i in enumerate(idx):
                pc, rgb, gt = pp.preprocess_on_device(pcs[j], rgbs[j], gts[gt_row[i]] if i in gt_row else None)
                img = prep.prepare_device_images(rgb[None])[0]
                cloud, depth, count = prep.prepare_device_clouds(pc[None])[0]
                mask = prep.prepare_device_masks(gt[None])[0] if gt is not None else None
                out.append((DeviceSample((img, cloud, depth), count), mask))
            return out

        with torch.cuda.device(prep.device):
            return scatter_by_shape([d[0] for d in dec], range(len(dec)), scans_of)

    def train(self):
        ds = self._train
        return self._items(len(ds), lambda i: self._decode(ds.img_paths[i], None), ds.labels)

    def test(self):
        ds = self._test
        return self._items(len(ds), lambda i: self._decode(ds.img_paths[i], ds.gt_paths[i] if ds.gt_paths[i] != 0 else None), ds.labels,
                           [str(p[0]) for p in ds.img_paths])


class PointCloudClass(_RawClassSource):
    """One class directory of UNORGANISED scans -- ``<class>/train/good/*.ply`` and ``<class>/test/<kind>/*.ply``, point lists with
    optional ``red green blue`` and, in a defect scan, a per-point integer ``label`` (0: sound) -- as the data object of
    evaluate.ClassRun / evaluate_classes, with MVTec3DClass's protocol.  Reader threads parse the files (utils.ply.read_points); every
    batch is one ``organize`` call (csrc/organize.hip; docs/organize.md) and SamplePrep's device entry points, and it yields, sample
    for sample and bit for bit, what MVTec3DClass with img_process_method='hip' yields over the tree ``python -m cmdiad_amd.organize``
    writes from this directory.  ``<class>/camera.json`` (optional) fixes the camera: ``{"kind": "orthographic", "x0", "y0", "pitch"
    [, "pitch_y"]}`` or ``{"kind": "pinhole", "fx", "fy", "cx", "cy"}``, with optional ``"T"`` (3 x 4), ``"size": [H, W]`` and ``"fill"``;
    without it every scan gets ``fit_orthographic`` at ``args.organize_size`` (default 448) squared with a margin of 1, and
    ``args.organize_fill`` (default 1).  Order and labels are TestDataset's (sorted directories, then sorted files; ``good`` is 0,
    anything else 1); a file without colours gives a black image, a good sample's mask is zeros, a defect scan without ``label``
    raises; ``rgb_path`` is the PLY's path.  There is no host path."""
    _no_host_path = ("PointCloudClass: unorganised scans are put on the pixel grid on the device only, there is no host path: "
                     "img_process_method must be 'hip', got {method!r} (or write the tree with python -m cmdiad_amd.organize and "
                     "read it with MVTec3DClass)")

    def __init__(self, dataset_path, class_name, args):
        import json
        from .organize import Camera
        super().__init__(class_name, args)
        root = Path(dataset_path, class_name)
        self.train_files = [str(p) for p in _sorted_glob(root, "train", "good", "*.ply")]
        self.test_files, self.test_labels = [], []
        test = Path(root, "test")
        for kind in sorted(os.listdir(test)) if test.is_dir() else []:
            files = [str(p) for p in _sorted_glob(test, kind, "*.ply")]
            self.test_files += files
            self.test_labels += [0 if kind == "good" else 1] * len(files)
        self.n_train, self.n_test = len(self.train_files), len(self.test_files)
        size = int(getattr(args, "organize_size", 448))
        self.camera, self.size, self.fill = None, (size, size), int(getattr(args, "organize_fill", 1))
        cam_path = Path(root, "camera.json")
        if cam_path.is_file():
            with open(cam_path) as f:
                c = json.load(f)
            if c.get("kind") == "orthographic":
                self.camera = Camera.orthographic(c["x0"], c["y0"], c["pitch"], c.get("pitch_y"), c.get("T"))
            elif c.get("kind") == "pinhole":
                self.camera = Camera.pinhole(c["fx"], c["fy"], c["cx"], c["cy"], c.get("T"))
            else:
                raise ValueError(f"{cam_path}: kind must be 'orthographic' or 'pinhole', got {c.get('kind')!r}")
            self.size = tuple(int(v) for v in c.get("size", self.size))
            self.fill = int(c.get("fill", self.fill))
            if len(self.size) != 2:
                raise ValueError(f"{cam_path}: size must be [H, W]")

    @staticmethod
    def decode(path, label):
        """(points float32 [N,3], colours uint8 [N,3] or None, labels uint8 [N] or None) of one file, on a reader thread"""
        import numpy as np
        from .utils import ply
        v = ply.read_points(path)
        pts = np.stack([v["x"], v["y"], v["z"]], axis=1)
        rgb = None
        if all(c in v and v[c].dtype == np.uint8 for c in ("red", "green", "blue")):
            rgb = np.stack([v["red"], v["green"], v["blue"]], axis=1)
        lab = None
        if label:
            if "label" not in v:
                raise ValueError(f"PointCloudClass: {path}: a defect scan needs a per-point integer 'label' property (0: sound)")
            lab = (v["label"] != 0).astype(np.uint8)
        return pts, rgb, lab

    def organize_batch(self, dec):
        """decoded scans -> the Organized of the batch: one upload of the three lists, one fit where there is no camera.json, one
        organize call"""
        import numpy as np
        from . import organize as og
        dev = self.sample_prep().device
        lengths = [len(d[0]) for d in dec]
        P = sum(lengths)
        any_rgb, any_lab = any(d[1] is not None for d in dec), any(d[2] is not None for d in dec)
        colors = np.concatenate([d[1] if d[1] is not None else np.zeros((len(d[0]), 3), np.uint8) for d in dec]) if any_rgb else None
        labels = np.concatenate([d[2] if d[2] is not None else np.zeros(len(d[0]), np.uint8) for d in dec]) if any_lab else None
        with torch.cuda.device(dev):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True) if a is not None else None
            points = up(np.concatenate([d[0] for d in dec]).reshape(P, 3))
            H, W = self.size
            cams = self.camera if self.camera is not None else og.fit_orthographic(points, lengths, H, W, margin=1)
            return og.organize(points, lengths, cams, H, W, self.fill, up(colors), up(labels))

    def _prepare(self, dec):
        """decoded scans -> [(DeviceSample, mask or None)]"""
        prep = self.sample_prep()
        org = self.organize_batch(dec)
        with torch.cuda.device(prep.device):
            imgs = prep.prepare_device_images(org.rgb)
            clouds = prep.prepare_device_clouds(org.xyz)
            masks = prep.prepare_device_masks(org.mask)
        return [(DeviceSample((imgs[j], clouds[j][0], clouds[j][1]), clouds[j][2]), masks[j] if dec[j][2] is not None else None)
                for j in range(len(dec))]

    def train(self):
        files = self.train_files
        return self._items(self.n_train, lambda i: self.decode(files[i], 0), [0] * self.n_train)

    def test(self):
        files, labels = self.test_files, self.test_labels
        return self._items(self.n_test, lambda i: self.decode(files[i], labels[i]), labels, files)


def dataset_classes(args):
    """{class name: data object} for evaluate_classes: the classes of args.dataset_type ('mvtec3d' default, 'eyecandies') that have a
    directory under args.dataset_path, in the reference's order (main.py:10-16).  An Eyecandies class directory with ``train/data`` is
    the raw download (EyecandiesRawClass); any other is a tree in MVTec 3D-AD's layout (MVTec3DClass) -- a tree the preprocessing
    script has cleaned, unless ``args.raw_scans`` says the MVTec 3D-AD tree is the raw download (MVTec3DRawClass: the scans are
    cleaned on the device as they are read)."""
    kind = getattr(args, "dataset_type", "mvtec3d")
    if kind not in ("mvtec3d", "eyecandies"):
        raise ValueError(f"dataset_type must be 'mvtec3d' or 'eyecandies', got {kind!r}")
    names = eyecandies_classes() if kind == "eyecandies" else mvtec3d_classes()

    def source(c):
        if kind == "mvtec3d" and getattr(args, "raw_scans", False):
            return MVTec3DRawClass(args.dataset_path, c, args)
        raw = kind == "eyecandies" and os.path.isdir(Path(args.dataset_path, c, "train", "data"))
        return (EyecandiesRawClass if raw else MVTec3DClass)(args.dataset_path, c, args)

    found = {c: source(c) for c in names if os.path.isdir(Path(args.dataset_path, c))}
    if not found:
        raise FileNotFoundError(f"no {kind} class directory under {args.dataset_path!r}")
    return found
