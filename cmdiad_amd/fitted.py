"""A fitted class in ONE file: the patch libraries, the six statistics and the two one-class SVMs of a method object after
``fit`` -- everything ``predict`` reads -- so that scoring needs neither the training set nor the fit (docs/fitted.md).

The format uses no pickle: reading a file never executes anything.

    offset 0      8-byte magic  b"CMDFIT\\0\\1"
           8      u32 format version (1), little-endian
           12     u32 header length in bytes
           16     header: UTF-8 JSON, zero-padded to a 4096-byte boundary
           ...    arrays: raw little-endian, C order, each starting on a 4096-byte boundary

The header names the method class, the class, every ``args`` field the scoring path reads, the search operand type, the content
digests of the backbones and of the head the fit was made with, and the array table (name, dtype, shape, offset, nbytes,
digest64; for 2-D arrays also the digests of their 128-row blocks, which is what lets a rank that reads only its row shard verify
it).  The digest is the one of ``cmdiad_digest64`` (include/cmdiad_hip.h); ``digest64_host`` restates it in numpy.  It guards
against mistakes -- another checkpoint, a damaged file, a wrong shard -- not against adversaries.

The first half of this module (write_file / read_header / read_array / digest64_host / restore_fuser) works on numpy alone and
needs no GPU; the second half (save / load / FittedClass, Bank.from_file's loader) moves the arrays to and from the device.
"""
import json
import os
import struct
import sys
import types

import numpy as np

MAGIC = b"CMDFIT\x00\x01"
VERSION = 1
ALIGN = 4096
MAX_HEADER = 1 << 20
BLOCK_ROWS = 128            # engine.shard_range cuts libraries on multiples of 128 rows: a shard is a whole number of blocks
DTYPES = {"float32": "<f4", "float64": "<f8", "int64": "<i8", "int32": "<i4", "uint8": "|u1", "uint64": "<u8"}
LIBRARIES = ("patch_xyz_lib", "patch_rgb_lib", "patch_fusion_lib")
STATS = ("xyz_mean", "xyz_std", "rgb_mean", "rgb_std", "fusion_mean", "fusion_std")
FUSERS = ("detect_fuser", "seg_fuser")
# every field of `args` that the scoring path (construction of the method object, extraction, normalisation, search, late fusion)
# reads; a field the namespace does not carry is stored as null
ARG_FIELDS = ("method_name", "rgb_backbone_name", "xyz_backbone_name", "group_size", "num_group", "rgb_size", "xyz_size", "gt_size",
              "main_modality", "use_hn", "use_hn_conv", "use_hn_from_rgb_mlp", "use_hn_from_rgb_conv", "use_hrnet", "use_uff",
              "use_depth", "c_hrnet", "xyz_s_lambda", "xyz_smap_lambda", "rgb_s_lambda", "rgb_smap_lambda", "fusion_s_lambda",
              "fusion_smap_lambda", "f_coreset", "coreset_eps", "coreset_dtype", "random_state", "ocsvm_nu", "ocsvm_maxiter",
              "memory_bank", "dist_method_s")
_MASK = 0xFFFFFFFFFFFFFFFF


class FitFileError(ValueError):
    """The file is not a fit file this version can read, or its content does not match its own header."""


class FitMismatch(ValueError):
    """The file is sound, but it was fitted with something else than the object it is loaded into."""


# ------------------------------------------------------------------------------------------------ digest (host restatement)
def _mix(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def digest64_host(array, seed=0):
    """cmdiad_digest64 in numpy: sum_i h(h(seed + i) ^ w_i) mod 2^64 over the little-endian 32-bit words w_i of the array's bytes
    (C order; a byte count that is no multiple of 4 is zero-padded, as ops.module_digest does) -> Python int."""
    raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
    if raw.size % 4:
        raw = np.concatenate([raw, np.zeros(4 - raw.size % 4, dtype=np.uint8)])
    words = raw.view("<u4")
    total, seed = 0, int(seed) & _MASK
    with np.errstate(over="ignore"):
        for lo in range(0, words.size, 1 << 20):            # bounded temporaries: 8 MiB per step
            w = words[lo:lo + (1 << 20)].astype(np.uint64)
            idx = np.arange(lo, lo + w.size, dtype=np.uint64) + np.uint64(seed)
            total = (total + int(_mix(_mix(idx) ^ w).sum(dtype=np.uint64))) & _MASK
    return total


def block_digests_host(array, block_rows=BLOCK_ROWS):
    """Digests of the blocks of `block_rows` rows of a 2-D array, block b seeded with its first word's index in the whole array:
    their sum mod 2^64 is digest64_host(array, 0), and the sum over a run of blocks is the digest of those rows at that offset."""
    a = np.ascontiguousarray(array)
    per_row = a.shape[1] * a.dtype.itemsize // 4
    return [digest64_host(a[lo:lo + block_rows], lo * per_row) for lo in range(0, a.shape[0], block_rows)]


def _blockable(shape, dtype):
    return len(shape) == 2 and shape[0] > 0 and (shape[1] * np.dtype(dtype).itemsize) % 4 == 0


# ------------------------------------------------------------------------------------------------ file
def _pad(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _dtype_name(dt):
    for name, code in DTYPES.items():
        if np.dtype(code) == np.dtype(dt):
            return name
    raise FitFileError(f"dtype: {np.dtype(dt)} is not one of {sorted(DTYPES)}")


def write_file(path, header, arrays, digests=None, blocks=None, fmt="cmdfit"):
    """Write `arrays` ({name: numpy array}) with `header` (a JSON-able dict; "format", "version" and "arrays" are filled in here;
    fmt: the header's "format", "cmdfit" for a fit -- other files in this container name their own, regions.py's calibration).
    digests / blocks: {name: int} / {name: [int]} already known (computed on the device); the others are computed on the host.
    Atomic: written under a temporary name in the same directory, flushed, then os.replace()d."""
    digests, blocks = digests or {}, blocks or {}
    table, items = [], []
    for name, a in arrays.items():
        a = np.asarray(a)
        dt = _dtype_name(a.dtype)
        a = np.ascontiguousarray(a, dtype=np.dtype(DTYPES[dt])).reshape(a.shape)      # (ascontiguousarray makes 0-dim 1-dim)
        entry = dict(name=str(name), dtype=dt, shape=[int(s) for s in a.shape], offset=0, nbytes=int(a.nbytes),
                     digest64=f"{(digests[name] if name in digests else digest64_host(a)) & _MASK:016x}")
        if _blockable(a.shape, a.dtype):
            bl = blocks[name] if name in blocks else block_digests_host(a)
            entry.update(block_rows=BLOCK_ROWS, block_digests=[f"{b & _MASK:016x}" for b in bl])
        table.append(entry)
        items.append(a)
    head = dict(header, format=fmt, version=VERSION, arrays=table)
    # the offsets depend on the header's length and are part of it: fixed-width placeholders first, then the real values
    for e in table:
        e["offset"] = 10 ** 15
    size = len(json.dumps(head).encode())
    if size > MAX_HEADER:
        raise FitFileError(f"{path}: header_len: a header of {size} bytes is above the limit of {MAX_HEADER}")
    pos = _pad(16 + size)
    for e in table:
        e["offset"] = pos
        pos = _pad(pos + e["nbytes"])
    blob = json.dumps(head).encode()
    assert len(blob) <= size
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            f.write(MAGIC + struct.pack("<II", VERSION, len(blob)) + blob)
            for e, a in zip(table, items):
                f.write(b"\0" * (e["offset"] - f.tell()))
                f.write(memoryview(a.reshape(-1)).cast("B") if a.size else b"")
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return head


def read_header(path):
    """The validated header of a fit file.  Everything is checked BEFORE any payload is touched: magic, version, header length,
    every array's dtype against the whitelist and its offset / nbytes against its shape and the file's size.  Every refusal is a
    FitFileError naming the file and the field."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        lead = f.read(16)
        if len(lead) < 16:
            raise FitFileError(f"{path}: magic: the file has {len(lead)} bytes, a fit file starts with 16")
        if lead[:8] != MAGIC:
            raise FitFileError(f"{path}: magic: {lead[:8]!r} is not {MAGIC!r}")
        version, hlen = struct.unpack("<II", lead[8:])
        if version != VERSION:
            raise FitFileError(f"{path}: version: format version {version}, this reader knows version {VERSION}")
        if hlen > MAX_HEADER:
            raise FitFileError(f"{path}: header_len: {hlen} bytes is above the limit of {MAX_HEADER}")
        if 16 + hlen > size:
            raise FitFileError(f"{path}: header_len: the header ends at byte {16 + hlen} of a file of {size} (truncated)")
        blob = f.read(hlen)
    try:
        head = json.loads(blob.decode("utf-8"))
    except ValueError as e:
        raise FitFileError(f"{path}: header: not UTF-8 JSON ({e})") from None
    if not isinstance(head, dict) or not isinstance(head.get("arrays"), list):
        raise FitFileError(f"{path}: arrays: the header has no array table")
    seen = set()
    for e in head["arrays"]:
        if not isinstance(e, dict) or not isinstance(e.get("name"), str) or e["name"] in seen:
            raise FitFileError(f"{path}: name: an array table entry without a name of its own")
        seen.add(e["name"])
        where = f"{path}: array {e['name']!r}"
        if e.get("dtype") not in DTYPES:
            raise FitFileError(f"{where}: dtype: {e.get('dtype')!r} is not one of {sorted(DTYPES)}")
        shape = e.get("shape")
        if not isinstance(shape, list) or not all(isinstance(s, int) and not isinstance(s, bool) and s >= 0 for s in shape):
            raise FitFileError(f"{where}: shape: {shape!r}")
        count = 1
        for s in shape:
            count *= s
        nbytes, offset = e.get("nbytes"), e.get("offset")
        if not isinstance(nbytes, int) or isinstance(nbytes, bool) or nbytes != count * np.dtype(DTYPES[e["dtype"]]).itemsize:
            raise FitFileError(f"{where}: nbytes: {nbytes!r} is not shape {shape} x {e['dtype']}")
        if not isinstance(offset, int) or isinstance(offset, bool) or offset % ALIGN or offset < _pad(16 + hlen):
            raise FitFileError(f"{where}: offset: {offset!r} is not a multiple of {ALIGN} behind the header")
        if offset + nbytes > size:
            raise FitFileError(f"{where}: offset: bytes [{offset}, {offset + nbytes}) lie outside a file of {size} (truncated)")
        try:
            int(e.get("digest64"), 16)
            bl = [int(b, 16) for b in e.get("block_digests", [])]
        except (TypeError, ValueError):
            raise FitFileError(f"{where}: digest64: not hexadecimal") from None
        if bl and (e.get("block_rows") != BLOCK_ROWS or len(shape) != 2 or len(bl) != (shape[0] + BLOCK_ROWS - 1) // BLOCK_ROWS):
            raise FitFileError(f"{where}: block_digests: {len(bl)} blocks of {e.get('block_rows')!r} rows for shape {shape}")
    return head


def array_entry(head, name, path="<header>"):
    for e in head["arrays"]:
        if e["name"] == name:
            return e
    raise FitFileError(f"{path}: arrays: no array named {name!r} (the file has {[e['name'] for e in head['arrays']]})")


def _row_range(e, rows, path):
    shape = e["shape"]
    if rows is None:
        return 0, (shape[0] if shape else 1), shape
    if not shape:
        raise FitFileError(f"{path}: array {e['name']!r}: rows: a 0-dim array has no rows")
    lo, hi = int(rows[0]), int(rows[1])
    if not 0 <= lo <= hi <= shape[0]:
        raise FitFileError(f"{path}: array {e['name']!r}: rows: [{lo}, {hi}) is outside its {shape[0]} rows")
    return lo, hi, [hi - lo] + shape[1:]


def pread_into(fd, view, offset, path="<file>", chunk=8 << 20):
    """Fill the writable byte buffer `view` from `fd` at `offset` with os.pread calls of at most `chunk` bytes."""
    view = memoryview(view).cast("B")
    done = 0
    while done < len(view):
        got = os.pread(fd, min(chunk, len(view) - done), offset + done)
        if not got:
            raise FitFileError(f"{path}: offset: the file ends at byte {offset + done}, {len(view) - done} bytes short (truncated)")
        view[done:done + len(got)] = got
        done += len(got)


def read_array(path, name, rows=None, head=None):
    """Array `name` of the file as a numpy array; rows=(lo, hi): only that row range, and only those bytes are read (os.pread)."""
    head = head or read_header(path)
    e = array_entry(head, name, path)
    lo, hi, shape = _row_range(e, rows, path)
    dt = np.dtype(DTYPES[e["dtype"]])
    out = np.empty(shape, dtype=dt)
    row_bytes = e["nbytes"] // e["shape"][0] if e["shape"] and e["shape"][0] else e["nbytes"]
    if out.nbytes:
        fd = os.open(path, os.O_RDONLY)
        try:
            pread_into(fd, out.reshape(-1).view(np.uint8), e["offset"] + lo * row_bytes, path)
        finally:
            os.close(fd)
    return out


def fuser_arrays(fuser, prefix):
    """The fitted state of a one-class SVM (scikit-learn's SGDOneClassSVM or ocsvm.DeviceSGDOneClassSVM) that scoring reads."""
    # in their own types: scikit-learn keeps coef_ / offset_ in the type of the rows it was fitted on (float32 from the score maps)
    return {f"{prefix}.coef_": np.asarray(fuser.coef_), f"{prefix}.offset_": np.asarray(fuser.offset_),
            f"{prefix}.n_iter_": np.asarray(int(fuser.n_iter_), dtype=np.int64)}


def restore_fuser(fuser, coef, offset, n_iter):
    """Put stored coef_ / offset_ / n_iter_ into an unfitted one-class SVM object: with n_features_in_ that is all score_samples
    (and multiple_features._score_samples' fast path) reads.  -> fuser"""
    coef = np.array(coef)
    fuser.coef_ = coef
    fuser.offset_ = np.array(offset).reshape(1)
    fuser.n_iter_ = int(n_iter)
    fuser.n_features_in_ = int(coef.shape[-1])
    return fuser


# ------------------------------------------------------------------------------------------------ device side
def device_digests(rows):
    """(digest, [block digests]) of a 2-D contiguous device tensor by cmdiad_digest64: one launch per 128-row block into a table on
    the device, ONE device-to-host read; the whole array's digest (seed 0) is the sum of its blocks'."""
    import torch
    from . import ops
    n = rows.shape[0]
    per_row = rows.shape[1] * rows.element_size() // 4
    table = torch.zeros(((n + BLOCK_ROWS - 1) // BLOCK_ROWS,), dtype=torch.int64, device=rows.device)
    for b, lo in enumerate(range(0, n, BLOCK_ROWS)):
        ops.digest64(rows[lo:lo + BLOCK_ROWS], lo * per_row, table[b:b + 1])
    bl = [int(v) & _MASK for v in table.cpu().tolist()]
    return sum(bl) & _MASK, bl


def rows_to_device(path, name, rows=None, device="cuda", verify=True, head=None, chunk_bytes=8 << 20):
    """Rows [lo, hi) (default: all) of the 2-D array `name`, streamed from the file to the device through two pinned buffers: the
    os.pread of chunk k + 1 runs beside the host-to-device copy of chunk k.  verify: the rows' digest is computed on the device
    and compared with the header's -- the whole array's, or for a row range the sum of its 128-row blocks' (the range must then
    start on a block boundary and end on one or at the last row, which every engine.shard_range does)."""
    import torch
    from . import ops
    head = head or read_header(path)
    e = array_entry(head, name, path)
    if len(e["shape"]) != 2:
        raise FitFileError(f"{path}: array {name!r}: shape: {e['shape']} is not a 2-D library")
    lo, hi, shape = _row_range(e, rows, path)
    tdt = getattr(torch, e["dtype"])
    out = torch.empty(shape, dtype=tdt, device=device)
    row_bytes = shape[1] * out.element_size()
    if hi > lo and row_bytes:
        step = max(1, chunk_bytes // row_bytes)
        pinned = [torch.empty((min(step, hi - lo), shape[1]), dtype=tdt, pin_memory=True) for _ in range(2)]
        free = [None, None]
        fd = os.open(path, os.O_RDONLY)
        try:
            for k, r in enumerate(range(lo, hi, step)):
                m = min(step, hi - r)
                buf = pinned[k % 2][:m]
                if free[k % 2] is not None:
                    free[k % 2].synchronize()           # the copy that last read this buffer is done
                pread_into(fd, buf.numpy().reshape(-1).view(np.uint8), e["offset"] + r * row_bytes, path)
                out[r - lo:r - lo + m].copy_(buf, non_blocking=True)
                free[k % 2] = torch.cuda.Event()
                free[k % 2].record()
        finally:
            os.close(fd)
            for ev in free:
                if ev is not None:
                    ev.synchronize()
    if verify and hi > lo:          # (an empty shard has nothing to verify)
        whole = lo == 0 and hi == e["shape"][0]
        if whole:
            want = int(e["digest64"], 16)
        else:
            if "block_digests" not in e:
                raise FitFileError(f"{path}: array {name!r}: block_digests: the file has none, a row range cannot be verified")
            if lo % BLOCK_ROWS or (hi % BLOCK_ROWS and hi != e["shape"][0]):
                raise FitFileError(f"{path}: array {name!r}: rows: [{lo}, {hi}) does not lie on {BLOCK_ROWS}-row blocks")
            want = sum(int(b, 16) for b in e["block_digests"][lo // BLOCK_ROWS:(hi + BLOCK_ROWS - 1) // BLOCK_ROWS]) & _MASK
        got = ops.digest_value(ops.digest64(out, lo * (row_bytes // 4)))
        if got != want:
            raise FitFileError(f"{path}: array {name!r}: digest64: rows [{lo}, {hi}) hash to {got:016x} on the device, the header "
                               f"says {want:016x} (the payload was changed or damaged)")
    return out


def weight_digests(method):
    """{'rgb_backbone', 'xyz_backbone', 'fusion'}: ops.module_digest of the weights the method object extracts and hallucinates with."""
    from . import ops
    ex = method.deep_feature_extractor
    fusion = getattr(method, "fusion", None)
    return dict(rgb_backbone=f"{ops.module_digest(ex.rgb_backbone):016x}", xyz_backbone=f"{ops.module_digest(ex.xyz_backbone):016x}",
                fusion=f"{ops.module_digest(fusion):016x}" if fusion is not None else None)


def _held(method, name):
    """What the method object holds under a lazy result attribute, without running a flush."""
    return method.__dict__.get("_lz_" + name)


def save(method, path):
    """method.save_fit(path): see multiple_features._MethodBase.save_fit."""
    import torch
    from . import ops
    method._flush("fit")
    method._flush("late")
    libs = {n: _held(method, n) for n in LIBRARIES if torch.is_tensor(_held(method, n))}
    if not libs:
        raise RuntimeError("save_fit: run_coreset has not run (the libraries are still per-sample lists)")
    multiple = getattr(method.args, "memory_bank", "multiple") == "multiple"
    if multiple and not all(hasattr(getattr(method, f), "coef_") for f in FUSERS):
        raise RuntimeError("save_fit: run_late_fusion has not run (memory_bank == 'multiple' needs the two fitted one-class SVMs)")
    arrays, digests, blocks = {}, {}, {}
    for n, lib in libs.items():
        rows = lib.detach().to(method.device, torch.float32).contiguous()
        digests[n], blocks[n] = device_digests(rows)
        arrays[n] = rows.cpu().numpy()
    stats = []
    for s in STATS:
        v = getattr(method, s)
        if torch.is_tensor(v):          # (a statistic this method never computes stays the constructor's 0 and is not stored)
            arrays[s] = np.asarray(v.detach().cpu().numpy(), dtype=np.float32).reshape(())
            stats.append(s)
    if multiple:
        for f in FUSERS:
            arrays.update(fuser_arrays(getattr(method, f), f))
    header = dict(method_class=type(method).__name__, class_name=method.class_name,
                  args={k: getattr(method.args, k, None) for k in ARG_FIELDS}, search_dtype=str(ops.SEARCH_DTYPE).replace("torch.", ""),
                  digests=weight_digests(method), stats=stats, n_train=int(method.__dict__.get("_fit_samples", 0)))
    write_file(path, header, arrays, digests, blocks)
    return path


def check_match(method, head, path):
    """FitMismatch naming the FIRST field in which the file and the method object differ: the class, a stored args field, a digest."""
    if head.get("method_class") != type(method).__name__:
        raise FitMismatch(f"{path}: method_class: fitted with {head.get('method_class')}, loaded into {type(method).__name__}")
    for k, v in head.get("args", {}).items():
        mine = getattr(method.args, k, None)
        if mine != v:
            raise FitMismatch(f"{path}: args.{k}: fitted with {v!r}, this object was built with {mine!r}")
    mine = weight_digests(method)
    for k in ("rgb_backbone", "xyz_backbone", "fusion"):
        if head.get("digests", {}).get(k) != mine[k]:
            raise FitMismatch(f"{path}: digests.{k}: the file was fitted with weights {head.get('digests', {}).get(k)}, this object's "
                              f"{k} weights hash to {mine[k]} on the device")


def load_into(method, path, verify=True):
    """method.load_fit(path, verify): see multiple_features._MethodBase.load_fit."""
    import torch
    head = read_header(path)
    check_match(method, head, path)
    names = {e["name"] for e in head["arrays"]}
    for n in LIBRARIES:
        if n in names:
            setattr(method, n, rows_to_device(path, n, None, method.device, verify, head))
    for s in head.get("stats", []):
        setattr(method, s, torch.from_numpy(read_array(path, s, head=head).reshape(())).to(method.device))
    if getattr(method.args, "memory_bank", "multiple") == "multiple":
        for f in FUSERS:
            restore_fuser(getattr(method, f), *(read_array(path, f"{f}.{a}", head=head) for a in ("coef_", "offset_", "n_iter_")))
    method.class_name = head.get("class_name")
    method.__dict__["_fit_samples"] = int(head.get("n_train", 0))
    method._banks = {}
    return head


def _method_classes():
    from .feature_extractors import multiple_features as mf
    return {c.__name__: c for c in (mf.RGBFeatures, mf.DepthFeatures, mf.PointFeatures, mf.DoubleRGBPointFeatures,
                                    mf.RGBorXYZWithOneHallucination, mf.RGBorXYZWithOneHallucinationFromFeature)}


def args_from_header(head):
    """The args namespace of a stored fit: evaluate.mtfi_args' defaults for the fields the file does not carry (none of them is
    read while scoring), every stored field on top."""
    from .evaluate import mtfi_args
    fields = dict(use_hn=False)
    fields.update({k: v for k, v in head.get("args", {}).items() if v is not None or k == "random_state"})
    return mtfi_args(**fields)


def load(path, args=None, extractor=None, verify=True):
    """A fresh method object of the stored class with the stored fit loaded.  args=None: the namespace is built from the header.
    extractor: the frozen backbones of another method object (Features(shared_extractor=...))."""
    head = read_header(path)
    classes = _method_classes()
    if head.get("method_class") not in classes:
        raise FitFileError(f"{path}: method_class: {head.get('method_class')!r} is not one of {sorted(classes)}")
    method = classes[head["method_class"]](args if args is not None else args_from_header(head), shared_extractor=extractor)
    method.load_fit(path, verify=verify)
    return method


class FittedClass:
    """A fit file opened for inference: the header now, the arrays when asked for."""

    def __init__(self, path):
        self.path, self.header = path, read_header(path)
        self.args = types.SimpleNamespace(**self.header.get("args", {}))
        self.class_name, self.method_class = self.header.get("class_name"), self.header.get("method_class")
        self._cache = {}

    def names(self):
        return [e["name"] for e in self.header["arrays"]]

    def array(self, name, rows=None):
        if rows is not None:
            return read_array(self.path, name, rows, self.header)
        if name not in self._cache:
            self._cache[name] = read_array(self.path, name, None, self.header)
        return self._cache[name]

    def stat(self, name):
        return float(self.array(name))

    def fuser(self, name):
        from sklearn.linear_model import SGDOneClassSVM
        a = self.args
        return restore_fuser(SGDOneClassSVM(random_state=42, nu=a.ocsvm_nu, max_iter=a.ocsvm_maxiter),
                             *(self.array(f"{name}.{k}") for k in ("coef_", "offset_", "n_iter_")))

    def workload(self):
        """'dino_pointmae' | 'mtfi' | None: the BatchPredictor workload that scores this fit."""
        a = self.args
        if self.method_class == "DoubleRGBPointFeatures" and not a.use_depth:
            return "dino_pointmae"
        if (self.method_class == "RGBorXYZWithOneHallucination" and a.use_hn and a.main_modality == "xyz"
                and not (a.use_hn_conv or a.use_hrnet or a.use_hn_from_rgb_mlp or a.use_hn_from_rgb_conv)):
            return "mtfi"
        return None

    def predictor(self, engine, batch=32, group=None, verify=True, replicate_f32=True, **kw):
        """A predictor.BatchPredictor over this fit ('mtfi' needs halluc=runtime.PackedHallucination(...) among **kw).  With a
        process group the search operands are the rank's row shard (replicate_f32=False: the fp32 rows too, read from disk as a
        shard).  The caller answers for `engine` holding the weights of the header's digests (load_fit checks them)."""
        from . import engine as eng
        from .predictor import BatchPredictor
        wl = self.workload()
        if wl is None:
            raise ValueError(f"{self.path}: a {self.method_class} fit (main_modality {self.args.main_modality!r}) has no BatchPredictor "
                             "workload; those are 'dino_pointmae' (DoubleRGBPointFeatures) and 'mtfi' (use_hn, main modality xyz)")
        rank, world = 0, 1
        if group is not None:
            import torch.distributed as td
            rank, world = td.get_rank(group), td.get_world_size(group)
        a, second = self.args, ("rgb" if wl == "dino_pointmae" else "fusion")
        banks = [eng.Bank.from_file(self.path, f"patch_{m}_lib", rank, world, replicate_f32, verify) for m in ("xyz", second)]
        stats = dict(xyz_mean=self.stat("xyz_mean"), xyz_std=self.stat("xyz_std"), rgb_mean=self.stat(f"{second}_mean"),
                     rgb_std=self.stat(f"{second}_std"))
        lambdas = (a.xyz_s_lambda, a.xyz_smap_lambda, getattr(a, f"{second}_s_lambda"), getattr(a, f"{second}_smap_lambda"))
        kw.setdefault("size", a.xyz_size)
        kw.setdefault("gt_size", a.gt_size)
        kw.setdefault("rgb_size", a.rgb_size)
        return BatchPredictor(engine, banks[0], banks[1], stats, self.fuser("detect_fuser"), self.fuser("seg_fuser"), lambdas=lambdas,
                              batch=batch, workload=wl, group=group, **kw)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2 or argv[0] != "info":
        print("usage: python -m cmdiad_amd.fitted info FILE", file=sys.stderr)
        return 2
    head = read_header(argv[1])
    print(json.dumps({k: v for k, v in head.items() if k != "arrays"}, indent=2, sort_keys=True))
    print(f"{'array':<24}{'dtype':<10}{'shape':<18}{'offset':>12}{'nbytes':>14}  digest64          blocks")
    for e in head["arrays"]:
        print(f"{e['name']:<24}{e['dtype']:<10}{str(tuple(e['shape'])):<18}{e['offset']:>12}{e['nbytes']:>14}  {e['digest64']}  "
              f"{len(e.get('block_digests', []))}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
