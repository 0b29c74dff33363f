"""Host model of ``block_nanmedian`` (mac-vo_amd/csrc/kp_select.hip) in plain Python / NumPy (TEST INFRASTRUCTURE), and the record populations the
selector's finishing pass is tested on.

The kernel finds the lower median of the non-NaN records by BUCKET REFINEMENT on order-preserving 32-bit keys inside an open-ended ``for (;;)``.  The model
restates that loop step by step — the keys, the min / max / count step and ``k = (cnt - 1) >> 1``, the shift ``s``, the 2048-bucket histogram and the owner
of rank ``k``, ``nlo`` / ``nhi``, and the switch to direct ranking at ``<= RANK_CAP`` keys with its ``(o < e) || (o == e && j < i)`` tie-break — so that its
termination and its result can be established on the CPU (tests/test_kp_median_host.py) before a population is given to a GPU
(tests/test_gpu_selector_finish.py).  It returns the median and the number of histogram rounds it took, and refuses to go past ``MAX_ROUNDS``.

Why the loop ends: a round maps the key span [lo, hi] onto 2048 buckets of 2^s keys, s = max(0, bits(span) - 11), and the next span lies inside one
bucket, so it has at most s bits: 32 -> 21 -> 10 -> 0.  With s = 0 a bucket is one key, the next range has lo == hi, and the loop returns at its head.
So at most three histograms are ever built; ``MAX_ROUNDS`` = 4 is the bound the tests assert."""
import numpy as np

RANK_CAP = 256
N_BUCKETS = 2048
NAN_KEY = 0xFFFFFFFF
MAX_ROUNDS = 4


def float_key(f):
    """Order-preserving float32 -> uint32 key (returned as int64); every NaN sorts last."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    u = f.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(f), NAN_KEY, key)


def key_float(k):
    k = int(k)
    u = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def _clz_int(span):
    """``__clz((int)span)`` of a 32-bit value: 0 once bit 31 is set (the cast makes it negative)."""
    assert 0 < span <= 0xFFFFFFFF
    return 32 - int(span).bit_length()


def nanmedian_twin(vals, max_rounds=MAX_ROUNDS):
    """(lower median of the non-NaN members as float32 — NaN when there are none —, histogram rounds taken).  ``vals`` in record order."""
    keys = float_key(np.asarray(vals).reshape(-1))
    live = keys != NAN_KEY
    cnt = int(live.sum())
    if cnt <= 0:
        return np.float32(np.nan), 0
    lo, hi = int(keys[live].min()), int(keys[live].max())
    k = (cnt - 1) >> 1
    rounds = 0
    while True:
        if lo == hi:
            return key_float(lo), rounds
        if rounds >= max_rounds:
            raise AssertionError(f"block_nanmedian model: more than {max_rounds} histogram rounds (lo={lo:#x}, hi={hi:#x}, k={k})")
        rounds += 1
        span = hi - lo
        s = max(0, 32 - _clz_int(span) - 11)
        assert (span >> s) < N_BUCKETS
        inside = keys[(keys >= lo) & (keys <= hi)]                  # a NaN key is above every hi
        hist = np.bincount((inside - lo) >> s, minlength=N_BUCKETS)
        assert hist.shape[0] == N_BUCKETS
        excl = np.cumsum(hist) - hist
        owner = np.nonzero((excl <= k) & (k < excl + hist))[0]
        assert owner.shape[0] == 1, "exactly one bucket owns rank k"
        b = int(owner[0])
        cb = int(hist[b])
        k = k - int(excl[b])
        nlo = lo + (b << s)
        w = ((1 << s) - 1) if s else 0
        nhi = hi if (hi - nlo) < w else nlo + w
        assert lo <= nlo <= nhi <= hi
        if cb <= RANK_CAP:
            lst = keys[(keys >= nlo) & (keys <= nhi)]               # the kernel's list is in whatever order its LDS atomics land; any order gives the same key
            assert lst.shape[0] == cb
            j = np.arange(cb)
            rank = ((lst[None, :] < lst[:, None]) | ((lst[None, :] == lst[:, None]) & (j[None, :] < j[:, None]))).sum(axis=1)
            hit = np.nonzero(rank == k)[0]
            assert hit.shape[0] == 1, "the ranks of a list are a permutation"
            return key_float(lst[hit[0]]), rounds
        lo, hi = nlo, nhi


# ---------------------------------------------------------------------------------------------------- populations
def _place(members, n_slots, rng):
    """``members`` at random slots of a NaN-filled float32 array of ``n_slots`` (a NaN slot is no record)."""
    members = np.asarray(members, dtype=np.float32)
    assert members.shape[0] <= n_slots and not np.isnan(members).any()
    assert not (np.signbit(members) & (members == 0)).any()       # torch.median does not define which of -0 / +0 it returns
    out = np.full(n_slots, np.nan, dtype=np.float32)
    out[rng.permutation(n_slots)[: members.shape[0]]] = members
    return out


def populations(n_slots, seed=0):
    """[(name, float32 [n_slots] with NaN = no member)]: what ``block_nanmedian`` has not met on the synthetic maps.  ``n_slots`` >= 1024."""
    assert n_slots >= 1024
    rng = np.random.default_rng(seed + n_slots)
    n = n_slots
    inf = np.float32(np.inf)
    pops = []
    add = lambda name, m: pops.append((name, _place(m, n_slots, rng)))  # noqa: E731
    add("constant", np.full(n, 0.75))
    add("two_values_60_40", np.where(np.arange(n) < (6 * n) // 10, 0.5, 2.0))               # > RANK_CAP ties at the rank: refined down to one key
    cluster = np.float32(1.0) + rng.integers(0, 4096, n - 2).astype(np.float32) * np.float32(2.0 ** -23)
    add("tight_cluster_with_outliers", np.concatenate([cluster, [np.float32(-1e30), inf]]))  # the first histogram puts the cluster in one bucket
    den = rng.integers(1, 1 << 20, n // 4).astype(np.uint32).view(np.float32)                # positive denormals
    rest = n - (n // 4 + n // 8 + n // 8 + n // 16)
    mixed = np.concatenate([den, -den[: n // 8], rng.normal(0, 1e-38, rest), rng.normal(0, 1.0, n // 8), np.zeros(n // 16)]).astype(np.float32)
    mixed = np.where(mixed == 0, np.float32(0.0), mixed)                                     # no -0
    add("mixed_signs_denormals", mixed)                                                      # key span >= 2^31: __clz((int)span) = 0
    add("majority_pos_inf", np.where(np.arange(n) < (6 * n) // 10, inf, rng.lognormal(0, 1, n).astype(np.float32)))
    add("majority_neg_inf", np.where(np.arange(n) < (6 * n) // 10, -inf, rng.lognormal(0, 1, n).astype(np.float32)))
    side = (n - 200) // 2
    mid = np.float32(1.0) + rng.integers(0, 8, 200 + (n - 200) % 2).astype(np.float32) * np.float32(2.0 ** -23)
    add("adjacent_keys_at_rank", np.concatenate([rng.uniform(0.001, 0.5, side), mid, rng.uniform(2.0, 100.0, side)]))   # direct ranking among duplicates
    base = rng.lognormal(0, 1.5, n).astype(np.float32)
    add("lognormal_n", base)
    add("lognormal_n_minus_1", base[:-1])                                                    # the other parity: one more NaN
    add("single_member", [3.5])
    add("two_members", [7.25, 0.125])
    return pops


def random_population(rng):
    """Mixed signs, denormals, duplicates, infinities, NaN gaps; 1 .. 6000 slots."""
    n = int(rng.integers(1, 6000))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        v = rng.normal(0, 10.0 ** rng.integers(-40, 30), n)
    elif kind == 1:
        v = rng.integers(1, 1 << 23, n).astype(np.uint32).view(np.float32).astype(np.float64) * rng.choice([-1.0, 1.0], n)     # denormals of both signs
    elif kind == 2:
        v = rng.choice(rng.normal(0, 1, int(rng.integers(1, 40))), n)                        # few distinct values: long runs of duplicates
    else:
        v = np.float32(rng.normal(0, 1)) + rng.integers(-300, 300, n).astype(np.float32) * np.float32(2.0 ** -24)
    with np.errstate(over="ignore"):
        v = np.asarray(v, dtype=np.float32)
    v = np.where(v == 0, np.float32(0.0), v)
    sel = rng.random(n)
    v = np.where(sel < 0.02, np.float32(np.inf), np.where(sel < 0.04, np.float32(-np.inf), v)).astype(np.float32)
    v[rng.random(n) < rng.choice([0.0, 0.1, 0.9])] = np.nan
    return v
