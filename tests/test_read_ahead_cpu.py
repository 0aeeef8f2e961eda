"""CPU: the host plumbing every loader shares -- cmdiad_amd.utils.batching.read_ahead (order, window, errors, shutdown) and
cmdiad_amd.dataset.epoch_batches (the epoch plan of FeatureRing and PairRing) against torch's DataLoader."""
import concurrent.futures as cf
import threading
import time
import types

import pytest
import torch

from cmdiad_amd.utils import batching


def _pool_threads():
    return {t for t in threading.enumerate() if t.name.startswith("ThreadPoolExecutor")}


@pytest.mark.parametrize("ahead", [1, 2, 4, 20])
@pytest.mark.parametrize("readers", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 5, 11])
def test_results_come_in_job_order_and_every_job_is_decoded_once(n, readers, ahead):
    """Early jobs take longest, so with more than one reader they finish last; the results still come in job order, one per job."""
    calls, lock = [], threading.Lock()

    def decode(job):
        time.sleep(0.0005 * (n - job))
        with lock:
            calls.append(job)
        return ("decoded", job)

    before = _pool_threads()
    got = list(batching.read_ahead(decode, range(n), readers, ahead))
    assert got == [("decoded", j) for j in range(n)]
    assert sorted(calls) == list(range(n))
    assert _pool_threads() <= before


@pytest.mark.parametrize("ahead", [1, 2, 4, 20])
@pytest.mark.parametrize("readers", [1, 3])
def test_never_more_than_ahead_results_outstanding(monkeypatch, readers, ahead):
    """Submissions counted at the pool: none before the first next() (a generator: its body has not started, which is within the
    `ahead` allowed), then the first min(ahead, n), and one more for every result taken: when result i is handed over exactly min(n, i + 1 + ahead) jobs have been submitted."""
    n, submitted = 11, []

    class CountingPool(cf.ThreadPoolExecutor):
        def submit(self, fn, *args, **kwargs):
            submitted.append(args[0])
            return super().submit(fn, *args, **kwargs)

    monkeypatch.setattr(batching, "cf", types.SimpleNamespace(ThreadPoolExecutor=CountingPool))
    gen = batching.read_ahead(lambda job: job * job, range(n), readers, ahead)
    assert submitted == []
    for i, result in enumerate(gen):
        assert result == i * i
        assert len(submitted) <= i + 1 + ahead and len(submitted) == min(n, i + 1 + ahead)
    assert submitted == list(range(n))


def test_a_decode_error_surfaces_at_its_job_and_the_pool_is_gone():
    def decode(job):
        if job == 3:
            raise KeyError("job 3")
        return job

    before = _pool_threads()
    gen = batching.read_ahead(decode, range(6), 2, 4)
    got = []
    with pytest.raises(KeyError, match="job 3"):
        for r in gen:
            got.append(r)
    assert got == [0, 1, 2]
    assert _pool_threads() <= before                 # shut down and joined: no live worker
    with pytest.raises(StopIteration):
        next(gen)


def test_closing_after_one_item_returns_and_the_pool_is_gone():
    before = _pool_threads()
    gen = batching.read_ahead(lambda job: job, range(50), 3, 4)
    assert next(gen) == 0
    gen.close()
    assert _pool_threads() <= before


def test_in_batches_cuts_and_finishes_the_iterable():
    assert list(batching.in_batches(iter(range(7)), 3)) == [[0, 1, 2], [3, 4, 5], [6]]
    assert list(batching.in_batches(iter(range(6)), 3)) == [[0, 1, 2], [3, 4, 5]]
    assert list(batching.in_batches(iter(()), 3)) == []
    before = _pool_threads()
    gen = batching.read_ahead(lambda job: job, range(6), 2, 3)
    assert list(batching.in_batches(gen, 3)) == [[0, 1, 2], [3, 4, 5]]
    assert _pool_threads() <= before                 # a full last batch too runs the generator to its end


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("batch", [1, 4, 10])
@pytest.mark.parametrize("n", [0, 1, 9, 10])
def test_epoch_batches_reproduce_dataloader_order(n, batch, shuffle, drop_last):
    """dataset.epoch_batches == the index batches of torch's DataLoader under the same global seed, two epochs, and the global RNG is
    in the same state afterwards (as many draws).  DataLoader refuses an empty dataset with shuffle=True, so that one cell has no
    independent yardstick: it only pins what the rings did before, an empty plan and the two draws of every other shuffled epoch
    (the loader's base seed and the sampler's seed)."""
    from torch.utils.data import DataLoader
    from cmdiad_amd.dataset import epoch_batches, epoch_length
    torch.manual_seed(3407)
    got = [epoch_batches(n, batch, shuffle, drop_last) for _ in range(2)]
    rng_after = torch.rand(1).item()
    torch.manual_seed(3407)
    if n == 0 and shuffle:
        want = [[], []]
        for _ in range(4):
            torch.empty((), dtype=torch.int64).random_()
    else:
        dl = DataLoader(list(range(n)), batch_size=batch, shuffle=shuffle, drop_last=drop_last)
        want = [[b.tolist() for b in dl] for _ in range(2)]
        assert epoch_length(n, batch, drop_last) == len(dl)
    assert got == want
    assert len(got[0]) == epoch_length(n, batch, drop_last)
    assert rng_after == torch.rand(1).item()
    if shuffle and n > 4 and got[0]:
        assert got[0] != got[1]                      # (the two epochs are two permutations)
