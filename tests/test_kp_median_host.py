"""CPU: the median select of the selector's finishing pass (``block_nanmedian``, restated in tests/kp_median_twin.py) on the populations the GPU tests
craft and on 200 random ones: the result is ``torch.median`` of the non-NaN members by value, and the refinement loop — open-ended in the kernel — ends
within ``MAX_ROUNDS`` histogram rounds.  This runs before any of these populations is given to a GPU: a population on which the model loops or disagrees
would be a finding about the kernel."""
import numpy as np
import pytest
import torch

from tests import kp_median_twin as T

SIZES = (48 * 64, 136 * 128)          # the two shapes tests/test_gpu_selector_finish.py runs the populations at


def _median_ref(v):
    m = v[~np.isnan(v)]
    return torch.from_numpy(m).median().item() if m.shape[0] else float("nan")


def _same(a, b):
    return (a == b) or (a != a and b != b)


def test_keys_preserve_order_and_round_trip():
    v = np.array([-np.inf, -1e30, -1.0, -1e-45, 0.0, 1e-45, 1e-38, 1.0, 1.0 + 2.0 ** -23, 3e38, np.inf], dtype=np.float32)
    k = T.float_key(v)
    assert (np.diff(k) > 0).all() and k.min() >= 0 and k.max() < T.NAN_KEY
    assert all(T.key_float(kk).view(np.uint32) == x.view(np.uint32) for kk, x in zip(k, v))
    assert T.float_key(np.array([np.nan, -np.nan], dtype=np.float32)).tolist() == [T.NAN_KEY] * 2
    assert T.float_key(np.array([-0.0], dtype=np.float32))[0] == T.float_key(np.array([0.0], dtype=np.float32))[0] - 1   # the one pair of equal values with two keys


@pytest.mark.parametrize("n_slots", SIZES)
def test_model_is_torch_median_on_the_crafted_populations(n_slots):
    rounds = {}
    for name, v in T.populations(n_slots):
        med, r = T.nanmedian_twin(v)
        assert _same(float(med), _median_ref(v)), (name, float(med), _median_ref(v))
        assert r <= T.MAX_ROUNDS, (name, r)
        rounds[name] = r
    assert len(rounds) == 11
    # the populations do what they were made for
    assert rounds["constant"] == 0 and rounds["single_member"] == 0         # lo == hi at the head of the loop
    assert rounds["two_values_60_40"] == 3                                  # > RANK_CAP ties: refined until a bucket is one key
    assert rounds["tight_cluster_with_outliers"] >= 2                       # the first histogram cannot split the cluster
    assert rounds["adjacent_keys_at_rank"] == 1 and rounds["two_members"] == 1
    keys = T.float_key(dict(T.populations(n_slots))["mixed_signs_denormals"])
    keys = keys[keys != T.NAN_KEY]
    assert int(keys.max() - keys.min()) >= 1 << 31                          # the span whose signed cast is negative


def test_model_is_torch_median_on_random_populations():
    rng = np.random.default_rng(7)
    seen = 0
    for i in range(200):
        v = T.random_population(rng)
        med, r = T.nanmedian_twin(v)
        assert _same(float(med), _median_ref(v)), (i, v.shape, float(med), _median_ref(v))
        assert r <= T.MAX_ROUNDS, (i, r)
        seen = max(seen, r)
    assert seen >= 2                                                        # more than one histogram round did occur


def test_model_refuses_to_loop():
    """The bound is checked, not assumed: with no round allowed the model raises instead of spinning."""
    with pytest.raises(AssertionError, match="histogram rounds"):
        T.nanmedian_twin(np.array([1.0, 2.0, 3.0], dtype=np.float32), max_rounds=0)
    assert T.nanmedian_twin(np.full(5, np.nan, dtype=np.float32))[1] == 0 and np.isnan(T.nanmedian_twin(np.full(5, np.nan, dtype=np.float32))[0])
