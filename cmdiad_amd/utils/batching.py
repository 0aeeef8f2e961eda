"""Host-side plumbing that dataset.py and the two preprocessing modules share: the decode-ahead loop of every loader
(dataset._device_items, utils.preprocessing.preprocess_dataset, utils.preprocessing_eyecandies.preprocess_dataset), and the
grouping of a batch's arrays by shape.  No torch.  (The pools of `read_ahead` end when its generator ends: a consumer that fails
between two results leaves the shutdown to the generator's close, which CPython runs as the consumer's frame unwinds.)"""
import concurrent.futures as cf
import itertools


def read_ahead(decode, jobs, readers, ahead):
    """Generator of ``decode(job)`` for every job, in job order.  The first ``min(ahead, n)`` jobs go to a pool of ``readers`` threads
    when the first result is asked for; every result taken submits exactly one further job before it is handed over, so there are
    never more than ``ahead`` results outstanding.  An exception of ``decode`` is raised at its job's position, after every earlier
    result.  The pool is shut down when the generator finishes, fails or is closed, and waits for the reads in flight (they are not
    cancelled)."""
    jobs = list(jobs)
    n = len(jobs)
    if ahead < 1:
        raise ValueError(f"read_ahead: ahead must be at least 1, got {ahead}")
    with cf.ThreadPoolExecutor(readers) as pool:
        reads = {i: pool.submit(decode, jobs[i]) for i in range(min(ahead, n))}
        nxt = len(reads)
        for i in range(n):
            result = reads.pop(i).result()
            if nxt < n:
                reads[nxt] = pool.submit(decode, jobs[nxt])
                nxt += 1
            yield result


def in_batches(items, batch):
    """Lists of up to ``batch`` consecutive items of an iterable; the last one may be shorter.  Runs the iterable to its end.  No
    reference to a list is kept once the consumer comes back for the next."""
    it = iter(items)
    while True:
        chunk = list(itertools.islice(it, batch))
        if not chunk:
            return
        yield chunk
        del chunk


def group_by_shape(arrays, indices, with_dtype=False):
    """{(H, W) or ((H, W), dtype name): [indices]} in order of first appearance: the members of a group share an upload and a launch."""
    import numpy as np
    from .png import RawImage
    from .tiff import RawCloud
    groups = {}
    for i in indices:
        a = arrays[i]
        a = a if isinstance(a, (RawCloud, RawImage)) else np.asarray(a)      # (a RawCloud / RawImage stands for the array its file holds)
        key = tuple(a.shape[:2])
        groups.setdefault((key, str(a.dtype)) if with_dtype else key, []).append(i)
    return groups


def scatter_by_shape(arrays, indices, call, with_dtype=False):
    """``call(key, idx)`` once per group of group_by_shape -> one result per member of idx, in idx's order.  Returns the results in
    the positions of ``arrays`` (None where an index was not asked for)."""
    res = [None] * len(arrays)
    for key, idx in group_by_shape(arrays, indices, with_dtype).items():
        for i, r in zip(idx, call(key, idx)):
            res[i] = r
    return res
