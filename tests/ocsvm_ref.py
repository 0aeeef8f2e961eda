"""Plain restatement of scikit-learn's float32 one-class SGD (linear_model/_sgd_fast.pyx.tp _plain_sgd32 with the hinge loss, the
L2 penalty, the 'optimal' schedule and one_class = 1; utils/_weight_vector.pyx.tp WeightVector32; utils/_seq_dataset.pyx.tp
ArrayDataset32.shuffle; utils/_random.pxd our_rand_r) -- the yardstick of cmdiad_ocsvm_fit (cmdiad_amd/csrc/ocsvm.hip).  Shared by
tests/test_gpu_ocsvm_edges.py and pinned to the installed scikit-learn by tests/test_ocsvm_ref_cpu.py.  No GPU, no cmdiad_amd import.

Nothing here needs a tolerance.  The doubles of the Cython sources are Python floats, its floats are Python floats rounded to
float32 after every operation (`_f32`): the product of two float32 values is exact in a double, a float32 quotient is the
correctly rounded double quotient rounded once more (53 >= 2 * 24 + 2 bits), and `w += val * (c / wscale)` IS a double sum stored
into a float.  The visiting order is the literal swap loop of ArrayDataset32.shuffle, run on the already permuted index array
every epoch -- not the parallel construction of cmdiad_amd/ocsvm.py, which the kernel shares.

The arithmetic, per sample at step t (t_ starts at 1), alpha = nu / 2:
    p      = float32(sum_f float32(w_f x_f) [in double] * wscale) + intercept          hit = p <= 1
    eta    = 1 / (alpha (optimal_init + t - 1));  wscale *= float32(max(0, 1 - eta alpha))
    if wscale < 1e-6:  w_f = float32(w_f float32(wscale)), wscale = 1                  the RESCALE
    if hit:            q = float32(float32(eta) / float32(wscale)), w_f = float32(double(w_f) + double(x_f) double(q))
    intercept += (eta if hit else 0) - 2 eta alpha
and coef_ = float32(w_f float32(wscale)) at the end.  wscale is a running product of factors that depend on t alone, so the steps
at which the rescale fires are data-independent (`rescale_steps`): the first one is step 681 755 for nu = 1.0, 1 829 034 for
nu = 0.5, 3 147 809 for nu = 0.3.

CASES (one table for the CPU pin and the GPU file).  `python -m pytest tests/test_ocsvm_ref_cpu.py -s` prints this table; a
rescale is given as step@position-in-epoch/lane-of-its-64-sample-chunk, `-` = the run ends before the first one, sub = float32
products w_f x_f that were subnormal.  The production-nu case is pinned to scikit-learn and to `rescale_steps` only (1.86 M steps
are not run through the Python loop), hence no counts.

rescale-lane0          n=2146   F=1 nu=1   tol=None   n_iter=320 hits=665638  misses=21082   rescale=681755@1472/0     sub=0
rescale-lane63         n=2009   F=2 nu=1   tol=None   n_iter=342 hits=646764  misses=40314   rescale=681755@703/63     sub=0
rescale-ragged         n=2228   F=3 nu=1   tol=None   n_iter=308 hits=686221  misses=3       rescale=681755@2214/38    sub=0
rescale-epoch-last     n=136351 F=4 nu=1   tol=None   n_iter=7   hits=843008  misses=111449  rescale=681755@136350/30  sub=0
rescale-epoch-first    n=340877 F=2 nu=1   tol=None   n_iter=5   hits=1616859 misses=87526   rescale=681755@0/0        sub=0
rescale-production-nu  n=50176  F=2 nu=0.5 tol=None   n_iter=37  hits=n/a     misses=n/a     rescale=1829034@22697/41  sub=n/a
stop-500x4             n=500    F=4 nu=0.5 tol=0.001  n_iter=8   hits=1998    misses=2002    rescale=-                 sub=0
stop-64x2              n=64     F=2 nu=0.5 tol=0.001  n_iter=14  hits=449     misses=447     rescale=-                 sub=0
stop-129x3             n=129    F=3 nu=0.5 tol=0.001  n_iter=11  hits=708     misses=711     rescale=-                 sub=0
stop-4096x2            n=4096   F=2 nu=0.5 tol=0.001  n_iter=7   hits=14337   misses=14335   rescale=-                 sub=0
stop-300x3             n=300    F=3 nu=0.5 tol=0.001  n_iter=9   hits=1349    misses=1351    rescale=-                 sub=0
stop-tol0              n=1000   F=2 nu=0.5 tol=0.0    n_iter=79  hits=39500   misses=39500   rescale=-                 sub=0
stop-tol0.1            n=1000   F=2 nu=0.5 tol=0.1    n_iter=6   hits=3001    misses=2999    rescale=-                 sub=0
stop-at-max-iter       n=129    F=3 nu=0.5 tol=0.001  n_iter=11  hits=708     misses=711     rescale=-                 sub=0
stop-max-iter-1        n=500    F=4 nu=0.5 tol=0.001  n_iter=1   hits=247     misses=253     rescale=-                 sub=0
stop-tol-none-7        n=64     F=2 nu=0.5 tol=None   n_iter=7   hits=225     misses=223     rescale=-                 sub=0
patience-1             n=500    F=4 nu=0.5 tol=0.001  n_iter=4   hits=998     misses=1002    rescale=-                 sub=0
patience-2             n=500    F=4 nu=0.5 tol=0.001  n_iter=5   hits=1247    misses=1253    rescale=-                 sub=0
patience-8             n=500    F=4 nu=0.5 tol=0.001  n_iter=11  hits=2749    misses=2751    rescale=-                 sub=0
n2-a                   n=2      F=1 nu=0.5 tol=0.001  n_iter=6   hits=4       misses=8       rescale=-                 sub=0
n2-b                   n=2      F=2 nu=0.5 tol=0.001  n_iter=7   hits=6       misses=8       rescale=-                 sub=0
n3-a                   n=3      F=2 nu=0.5 tol=0.001  n_iter=6   hits=5       misses=13      rescale=-                 sub=0
n3-b                   n=3      F=3 nu=0.5 tol=0.001  n_iter=6   hits=5       misses=13      rescale=-                 sub=0
n63-a                  n=63     F=3 nu=0.5 tol=0.001  n_iter=6   hits=144     misses=234     rescale=-                 sub=0
n63-b                  n=63     F=4 nu=0.5 tol=0.001  n_iter=14  hits=441     misses=441     rescale=-                 sub=0
n64-a                  n=64     F=4 nu=0.5 tol=0.001  n_iter=6   hits=126     misses=258     rescale=-                 sub=0
n64-b                  n=64     F=1 nu=0.5 tol=0.001  n_iter=12  hits=383     misses=385     rescale=-                 sub=0
n65-a                  n=65     F=1 nu=0.5 tol=0.001  n_iter=6   hits=182     misses=208     rescale=-                 sub=0
n65-b                  n=65     F=2 nu=0.5 tol=0.001  n_iter=14  hits=455     misses=455     rescale=-                 sub=0
n66-a                  n=66     F=2 nu=0.5 tol=0.001  n_iter=6   hits=164     misses=232     rescale=-                 sub=0
n66-b                  n=66     F=3 nu=0.5 tol=0.001  n_iter=17  hits=561     misses=561     rescale=-                 sub=0
n127-a                 n=127    F=3 nu=0.5 tol=0.001  n_iter=6   hits=302     misses=460     rescale=-                 sub=0
n127-b                 n=127    F=4 nu=0.5 tol=0.001  n_iter=16  hits=1015    misses=1017    rescale=-                 sub=0
n128-a                 n=128    F=4 nu=0.5 tol=0.001  n_iter=6   hits=270     misses=498     rescale=-                 sub=0
n128-b                 n=128    F=1 nu=0.5 tol=0.001  n_iter=9   hits=576     misses=576     rescale=-                 sub=0
n129-a                 n=129    F=1 nu=0.5 tol=0.001  n_iter=6   hits=375     misses=399     rescale=-                 sub=0
n129-b                 n=129    F=2 nu=0.5 tol=0.001  n_iter=11  hits=706     misses=713     rescale=-                 sub=0
n16384-a               n=16384  F=2 nu=0.5 tol=0.001  n_iter=6   hits=47913   misses=50391   rescale=-                 sub=0
n16384-b               n=16384  F=3 nu=0.5 tol=0.001  n_iter=7   hits=57343   misses=57345   rescale=-                 sub=0
n16385-a               n=16385  F=3 nu=0.5 tol=0.001  n_iter=6   hits=45706   misses=52604   rescale=-                 sub=0
n16385-b               n=16385  F=4 nu=0.5 tol=0.001  n_iter=7   hits=57346   misses=57349   rescale=-                 sub=0
n16386-a               n=16386  F=4 nu=0.5 tol=0.001  n_iter=6   hits=43544   misses=54772   rescale=-                 sub=0
n16386-b               n=16386  F=1 nu=0.5 tol=0.001  n_iter=6   hits=49158   misses=49158   rescale=-                 sub=0
n16449-a               n=16449  F=1 nu=0.5 tol=0.001  n_iter=6   hits=49115   misses=49579   rescale=-                 sub=0
n16449-b               n=16449  F=2 nu=0.5 tol=0.001  n_iter=7   hits=57571   misses=57572   rescale=-                 sub=0
seed-0                 n=1000   F=3 nu=0.5 tol=0.001  n_iter=8   hits=3996    misses=4004    rescale=-                 sub=0
seed-1                 n=1000   F=3 nu=0.5 tol=0.001  n_iter=8   hits=4000    misses=4000    rescale=-                 sub=0
seed-7                 n=1000   F=3 nu=0.5 tol=0.001  n_iter=7   hits=3500    misses=3500    rescale=-                 sub=0
seed-42                n=1000   F=3 nu=0.5 tol=0.001  n_iter=8   hits=3997    misses=4003    rescale=-                 sub=0
seed-12345             n=1000   F=3 nu=0.5 tol=0.001  n_iter=8   hits=4000    misses=4000    rescale=-                 sub=0
seed-2147483646        n=1000   F=3 nu=0.5 tol=0.001  n_iter=8   hits=4002    misses=3998    rescale=-                 sub=0
seed-instance          n=1000   F=3 nu=0.5 tol=0.001  n_iter=8   hits=4000    misses=4000    rescale=-                 sub=0
data-zeros             n=1000   F=3 nu=0.5 tol=0.001  n_iter=7   hits=3500    misses=3500    rescale=-                 sub=0
data-negative          n=1000   F=2 nu=0.5 tol=0.001  n_iter=6   hits=2788    misses=3212    rescale=-                 sub=0
data-centred           n=1000   F=2 nu=0.5 tol=0.001  n_iter=7   hits=3501    misses=3499    rescale=-                 sub=0
data-x1e3              n=1000   F=2 nu=0.5 tol=0.001  n_iter=6   hits=1       misses=5999    rescale=-                 sub=0
data-x1e-20            n=1000   F=2 nu=0.5 tol=0.001  n_iter=7   hits=3500    misses=3500    rescale=-                 sub=204
data-x1e-22            n=1000   F=2 nu=0.5 tol=0.001  n_iter=7   hits=3500    misses=3500    rescale=-                 sub=13998
data-x1e19             n=1000   F=2 nu=0.5 tol=0.001  n_iter=6   hits=1       misses=5999    rescale=-                 sub=0
data-same-rows         n=1000   F=2 nu=0.5 tol=0.001  n_iter=7   hits=1472    misses=5528    rescale=-                 sub=0
data-one-outlier       n=1000   F=2 nu=0.5 tol=0.001  n_iter=6   hits=1260    misses=4740    rescale=-                 sub=0
"""
import collections
import ctypes
import math

import numpy as np

MAX_INT32 = np.iinfo(np.int32).max
RESET_WSCALE_THRESHOLD = 1e-6         # utils/_weight_vector.pyx.tp, float32 instantiation
F32_TINY = float(np.finfo(np.float32).tiny)
CHUNK = 64                            # samples per step of ocsvm_epoch_kernel (one wave: the lanes prepare what depends on t alone)
FY_THREAD, FY_BLOCK = 64, 64 * 256    # generator steps per thread / per block of fy_targets_kernel (it counts n - 1 steps, not n)

_cf = ctypes.c_float()


def _f32(v):
    """A Python float rounded to float32 (round to nearest even, subnormals kept, overflow to inf), as a Python float."""
    _cf.value = v
    return _cf.value


# ================================================================================================ the shuffle
def xorshift32(s):
    s ^= (s << 13) & 0xFFFFFFFF
    s ^= s >> 17
    s ^= (s << 5) & 0xFFFFFFFF
    return s


def sgd_seed(random_state):
    """_fit_one_class: seed = check_random_state(self.random_state).randint(0, np.iinfo(np.int32).max) -- the only draw of a fit."""
    from sklearn.utils import check_random_state
    return int(check_random_state(random_state).randint(0, MAX_INT32))


def swap_targets(n, seed):
    """j_i of `for i in range(n - 1): j = i + our_rand_r(&seed) % (n - i)`; shuffle takes the seed by value, so every epoch draws
    the same targets.  our_rand_r replaces a zero state by 1."""
    s = seed or 1
    out = []
    for i in range(n - 1):
        s = xorshift32(s)
        out.append(i + (s & 0x7FFFFFFF) % (n - i))
    return out


def shuffle_in_place(order, targets):
    for i, j in enumerate(targets):
        order[i], order[j] = order[j], order[i]


# ================================================================================================ what depends on t alone
def _optimal_init(alpha):
    typw = math.sqrt(1.0 / math.sqrt(alpha))
    initial_eta0 = typw / max(1.0, -1.0)          # Hinge.cy_gradient(1.0, -typw) = -1
    return 1.0 / (initial_eta0 * alpha)


def _schedule(alpha, t_first, count):
    """For the steps t_first .. t_first + count - 1 (float64 arrays): eta, the float32 scale factor, float32(eta), and the two
    possible intercept updates.  numpy's float64 elementwise arithmetic is the IEEE arithmetic of the C doubles."""
    t = np.arange(t_first, t_first + count, dtype=np.float64)
    eta = 1.0 / (alpha * (_optimal_init(alpha) + t - 1.0))
    sc = np.maximum(0.0, 1.0 - ((1.0 - 0.0) * eta * alpha)).astype(np.float32).astype(np.float64)
    c = eta.astype(np.float32).astype(np.float64)
    two_eta_alpha = 2.0 * eta * alpha
    return eta, sc, c, eta - two_eta_alpha, 0.0 - two_eta_alpha


def rescale_steps(nu, T):
    """The steps t in 1 .. T (global, 1-based = t_ before the step's increment) at which `wscale < 1e-6` fires.  wscale is the
    sequential product of the float32-rounded factors since the last reset: np.multiply.accumulate multiplies in that order."""
    sc = _schedule(nu / 2.0, 1, T)[1]
    out, start = [], 0
    while start < T:
        below = np.nonzero(np.multiply.accumulate(sc[start:]) < RESET_WSCALE_THRESHOLD)[0]
        if len(below) == 0:
            break
        start += int(below[0]) + 1
        out.append(start)
    return out


# ================================================================================================ the fit
Stats = collections.namedtuple("Stats", "hits misses rescales sumloss counter stop subnormal t")
Stats.__doc__ = """hits / misses: samples with p <= 1 / p > 1, all epochs.  rescales: [(global step, in-epoch position)], position 0-based.
sumloss: per epoch.  counter: no_improvement_count after every epoch.  stop: 'rule' or 'max_iter'.  subnormal: float32 products
w_f x_f with 0 < |.| < 2^-126.  t: t_ after the fit (1 + n_iter n)."""


def fit(X, nu, max_iter, tol, random_state, n_iter_no_change=5, rescale=True, seed=None):
    """-> coef [F] float32, offset (float), n_iter, Stats.  rescale=False leaves the `wscale < 1e-6` branch out (what a kernel
    that mishandles it might compute): wscale just keeps shrinking.  seed: the uint32 handed to the shuffle as it is, instead of the
    one drawn from random_state (no random_state draws 0; the C entry point can be given it)."""
    X = np.asarray(X)
    assert X.dtype == np.float32 and X.ndim == 2 and X.shape[0] >= 2
    n, F = X.shape
    rows = X.astype(np.float64).tolist()
    alpha = nu / 2.0
    tol = -math.inf if tol is None else float(tol)
    targets = swap_targets(n, sgd_seed(random_state) if seed is None else seed)
    order = list(range(n))
    w, wscale, intercept, t = [0.0] * F, 1.0, 1.0, 1
    best_loss, counter, epoch, stop = math.inf, 0, 0, "max_iter"
    hits = misses = subnormal = 0
    rescales, losses, counters = [], [], []
    feats = range(F)
    f32 = _f32
    for epoch in range(max_iter):
        shuffle_in_place(order, targets)
        _, sc_e, c_e, hit_e, miss_e = (a.tolist() for a in _schedule(alpha, t, n))
        sumloss = 0.0
        for pos in range(n):
            x = rows[order[pos]]
            innerprod = 0.0
            for f in feats:
                pr = f32(w[f] * x[f])
                if pr != 0.0 and -F32_TINY < pr < F32_TINY:
                    subnormal += 1
                innerprod += pr
            innerprod *= wscale
            p = f32(innerprod) + intercept
            hit = p <= 1.0
            if hit:
                sumloss += 1.0 - p
            wscale *= sc_e[pos]
            if rescale and wscale < RESET_WSCALE_THRESHOLD:
                ws = f32(wscale)
                for f in feats:
                    w[f] = f32(w[f] * ws)
                wscale = 1.0
                rescales.append((t + pos, pos))
            if hit:
                ws = f32(wscale)
                q = f32(c_e[pos] / ws) if ws != 0.0 else math.inf
                for f in feats:
                    w[f] = f32(w[f] + x[f] * q)
                intercept += hit_e[pos]
                hits += 1
            else:
                intercept += miss_e[pos]
                misses += 1
        t += n
        losses.append(sumloss)
        if not (math.isfinite(intercept) and all(math.isfinite(v) for v in w)):
            raise ValueError("Floating-point under-/overflow occurred at epoch #%d." % (epoch + 1))
        if tol > -math.inf and sumloss > best_loss - tol * n:
            counter += 1
        else:
            counter = 0
        counters.append(counter)
        if sumloss < best_loss:
            best_loss = sumloss
        if counter >= n_iter_no_change:
            stop = "rule"
            break
    ws = f32(wscale)
    coef = np.array([f32(v * ws) for v in w], dtype=np.float32)
    return coef, 1.0 - intercept, epoch + 1, Stats(hits, misses, rescales, losses, counters, stop, subnormal, 1.0 + (epoch + 1) * n)


# ================================================================================================ fixtures
def score_like(n, F, seed):
    """Rows shaped like the late fusion's s_lib / s_map_lib (tests/test_gpu_ocsvm.py): positive scores of F banks, a few outliers."""
    g = np.random.default_rng(seed)
    x = np.abs(g.normal(1.0, 0.25, size=(n, F))).astype(np.float32)
    x[g.integers(0, n, max(1, n // 50))] *= 3.0
    return x


def centred(n, F, seed):
    """Zero-centred unit normal rows: no separating direction, so the loss keeps wandering and the stopping rule fires late."""
    return np.random.default_rng(seed).normal(0.0, 1.0, size=(n, F)).astype(np.float32)


def same_rows(n, F, seed):
    return np.tile(score_like(1, F, seed), (n, 1))


def same_rows_one_outlier(n, F, seed):
    x = same_rows(n, F, seed)
    x[n // 3] *= np.float32(-4.0)        # on the other side of the origin: p < 1 whatever the weights are, so it always updates them
    return x


def zeros(n, F, seed):
    return np.zeros((n, F), dtype=np.float32)


GENERATORS = {f.__name__: f for f in (score_like, centred, same_rows, same_rows_one_outlier, zeros)}

Case = collections.namedtuple("Case", "name group data n F scale nu max_iter tol rs n_iter_no_change")
RNG_INSTANCE = "RandomState"          # rs = (RNG_INSTANCE, k): a fresh np.random.RandomState(k) for every fit, on both sides
NU1_FIRST_RESCALE = 681755            # rescale_steps(1.0, ...)[0]; tests/test_ocsvm_ref_cpu.py checks the three constants
NU05_FIRST_RESCALE = 1829034
NU03_FIRST_RESCALE = 3147809


def _case(name, group, data, n, F, rs, scale=1.0, nu=0.5, max_iter=1000, tol=1e-3, ninc=5):
    return Case(name, group, data, n, F, scale, nu, max_iter, tol, rs, ninc)


def _rescale_case(name, data, n, F, rs):
    return _case(name, "rescale", data, n, F, rs, nu=1.0, max_iter=-(-NU1_FIRST_RESCALE // n) + 2, tol=None)


BOUNDARY_N = (2, 3, 63, 64, 65, 66, 127, 128, 129, 16384, 16385, 16386, 16449)

CASES = [
    # ---- the rescale at step 681 755 (nu = 1.0), by its place in ocsvm_epoch_kernel's 64-sample chunks; 5 * 136 351 = 681 755 and
    # 2 * 340 877 = 681 754 are the only divisors of usable size, so the epoch-boundary positions exist once each
    _rescale_case("rescale-lane0", "score_like", 2146, 1, 42),               # position 1472 = 23 * 64, a full chunk
    _rescale_case("rescale-lane63", "score_like", 2009, 2, 7),               # position 703 = 10 * 64 + 63
    _rescale_case("rescale-ragged", "centred", 2228, 3, 0),                  # position 2214 of 2228: lane 38 of the last chunk (52 samples)
    _rescale_case("rescale-epoch-last", "score_like", 136351, 4, 12345),     # position n - 1 of epoch 5: the rescaled state crosses a launch
    _rescale_case("rescale-epoch-first", "score_like", 340877, 2, 1),           # position 0 of epoch 3
    # the late fusion's own setting: nu = 0.5 at the row count of one image; 37 * 50 176 = 1 856 512 > 1 829 034
    _case("rescale-production-nu", "rescale", "score_like", 50176, 2, 42, nu=0.5, max_iter=37, tol=None),
    # ---- the stopping rule beyond "five non-improving epochs straight after the first"
    _case("stop-500x4", "stop", "centred", 500, 4, 42),
    _case("stop-64x2", "stop", "centred", 64, 2, 42),
    _case("stop-129x3", "stop", "centred", 129, 3, 42),
    _case("stop-4096x2", "stop", "centred", 4096, 2, 42),
    _case("stop-300x3", "stop", "centred", 300, 3, 7),
    _case("stop-tol0", "stop", "centred", 1000, 2, 42, tol=0.0),
    _case("stop-tol0.1", "stop", "centred", 1000, 2, 42, tol=0.1),
    _case("stop-at-max-iter", "stop", "centred", 129, 3, 42, max_iter=11),   # = n_iter_ of stop-129x3: the rule and max_iter coincide
    _case("stop-max-iter-1", "stop", "centred", 500, 4, 42, max_iter=1),
    _case("stop-tol-none-7", "stop", "centred", 64, 2, 42, max_iter=7, tol=None),
    # ---- n_iter_no_change: DeviceSGDOneClassSVM has the argument, scikit-learn's class does not -> held to `fit` above only
    _case("patience-1", "patience", "centred", 500, 4, 42, ninc=1),
    _case("patience-2", "patience", "centred", 500, 4, 42, ninc=2),
    _case("patience-8", "patience", "centred", 500, 4, 42, ninc=8),
] + [
    # ---- n on the kernels' own boundaries: the 64-sample chunk, 64 generator steps per thread and 16 384 per block (n - 1 steps)
    _case("n%d-%s" % (n, "ab"[k]), "boundary", ("score_like", "centred")[k], n, 1 + (i + k) % 4, (3, 11)[k])
    for i, n in enumerate(BOUNDARY_N) for k in (0, 1)
] + [
    _case("seed-%s" % rs, "seed", "centred", 1000, 3, rs) for rs in (0, 1, 7, 42, 12345, 2 ** 31 - 2)
] + [
    _case("seed-instance", "seed", "centred", 1000, 3, (RNG_INSTANCE, 99)),
    # ---- other data than positive scores
    _case("data-zeros", "data", "zeros", 1000, 3, 42),                       # coef_ stays exactly 0, only the intercept moves
    _case("data-negative", "data", "score_like", 1000, 2, 42, scale=-1.0),
    _case("data-centred", "data", "centred", 1000, 2, 5),
    _case("data-x1e3", "data", "score_like", 1000, 2, 42, scale=1e3),
    _case("data-x1e-20", "data", "score_like", 1000, 2, 42, scale=1e-20),    # w x ~ 1e-40: subnormal float32 products
    _case("data-x1e-22", "data", "score_like", 1000, 2, 42, scale=1e-22),    # w x ~ 1e-44: a few bits above the smallest subnormal
    _case("data-x1e19", "data", "score_like", 1000, 2, 42, scale=1e19),      # finite: coef_ ~ 6e15, p ~ 1e35
    _case("data-same-rows", "data", "same_rows", 1000, 2, 42),
    _case("data-one-outlier", "data", "same_rows_one_outlier", 1000, 2, 42),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
LOOP_FREE = ("rescale-production-nu",)    # pinned to scikit-learn and rescale_steps only


def make_X(case):
    x = GENERATORS[case.data](case.n, case.F, case.n + case.F)
    return np.ascontiguousarray(x * np.float32(case.scale)) if case.scale != 1.0 else x


def random_state(case):
    rs = case.rs
    return np.random.RandomState(rs[1]) if isinstance(rs, tuple) and rs[0] == RNG_INSTANCE else rs


def queries(case):
    """64 rows to score with a fitted model: the case's own kind of data, other rows."""
    x = GENERATORS[case.data](64, case.F, 3) if case.data != "zeros" else score_like(64, case.F, 3)
    return np.ascontiguousarray(x * np.float32(case.scale))


def run(case, rescale=True):
    return fit(make_X(case), case.nu, case.max_iter, case.tol, random_state(case), case.n_iter_no_change, rescale=rescale)


def table_line(case, n_iter, stats):
    """One line of the module docstring's table; stats = None for a LOOP_FREE case (its rescale from `rescale_steps`)."""
    if stats is None:
        steps = rescale_steps(case.nu, case.max_iter * case.n)
        res = ",".join("%d@%d/%d" % (s, (s - 1) % case.n, ((s - 1) % case.n) % CHUNK) for s in steps) or "-"
        hits = misses = sub = "n/a"
    else:
        res = ",".join("%d@%d/%d" % (s, p, p % CHUNK) for s, p in stats.rescales) or "-"
        hits, misses, sub = stats.hits, stats.misses, stats.subnormal
    return "%-22s n=%-6d F=%d nu=%-3g tol=%-6s n_iter=%-3d hits=%-7s misses=%-7s rescale=%-17s sub=%s" % (
        case.name, case.n, case.F, case.nu, case.tol, n_iter, hits, misses, res, sub)


def sklearn_fit(case, X=None):
    """The installed scikit-learn on the case's rows (n_iter_no_change = 5 only: SGDOneClassSVM has no such argument)."""
    import warnings
    from sklearn.linear_model import SGDOneClassSVM
    assert case.n_iter_no_change == 5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # ConvergenceWarning where max_iter ends the fit
        return SGDOneClassSVM(nu=case.nu, max_iter=case.max_iter, tol=case.tol, random_state=random_state(case)).fit(make_X(case) if X is None else X)
