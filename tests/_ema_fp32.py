"""The reference's ``ExponentialMovingAverage.update`` (lib/model/ema.py:25-44) restated in numpy float32, as torch's CPU kernels evaluate
``s.sub_(one_minus_decay * (s - p))``: the effective decay and ``one_minus_decay`` in Python double, then three fp32 operations, each
rounded once -- d = fl(s - p), t = fl(fl32(omd) * d), s' = fl(s - t).  tests/golden/make_golden_ema.py asserts that the class equals
this formula on every element before it writes tests/golden/golden_ema.npz.  TEST INFRASTRUCTURE ONLY: nothing here imports vpho_amd."""
import numpy as np

SIZES = (1, 3, 1023, 1024, 1025, 2048, 4099)                      # below, at and above the 1024 elements a block owns; odd tails
DECAYS = (0.999, 0.5)                                             # warm-up branch throughout | min() switches to `decay` at update 8
UPDATES = 12
KEPT = (1, 2, 8, 12)                                              # the updates after which the fixture keeps the shadows


def one_minus_decay(decay, num_updates):
    """-> (one_minus_decay of the update that makes the count num_updates + 1, that count); num_updates None: the fixed decay"""
    if num_updates is not None:
        num_updates += 1
        decay = min(decay, (1 + num_updates) / (10 + num_updates))
    return 1.0 - decay, num_updates


def update(s, p, omd):
    """one update of one tensor: float32 arrays s, p and the Python double omd -> the new float32 shadow"""
    assert s.dtype == np.float32 and p.dtype == np.float32
    with np.errstate(invalid='ignore', over='ignore'):
        d = (s - p).astype(np.float32)
        t = (np.float32(omd) * d).astype(np.float32)
        return (s - t).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """bit for bit: -0.0 differs from 0.0, a NaN equals a NaN of the same payload"""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())
