"""The reference's ``ExponentialMovingAverage`` (lib/model/ema.py, imported by its path: the class needs nothing but torch) run on the CPU
over seven tensors for twelve updates with new parameter values each time, for two decays, written to tests/golden/golden_ema.npz:
the start shadows, the parameters of every update, the shadows after updates 1, 2, 8 and 12, ``one_minus_decay`` of every update and
the keys of the class's ``state_dict()``.  One NaN and one +inf are planted in the parameters of update 2 (in the 1025-element tensor:
the inf in its first, whole block, the NaN in its one-element tail), so the kept shadows show them arriving (update 2) and what later
updates make of them (8, 12: the inf has become inf - inf).  Before anything is written the class must equal the three-rounding numpy
formula of tests/_ema_fp32.py on every element, bit for bit.  Run in the build container only."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import _ema_fp32 as EF  # noqa: E402

PLANT_UPDATE, PLANT_TENSOR, INF_AT, NAN_AT = 2, EF.SIZES.index(1025), 5, 1024


def reference_class():
    spec = importlib.util.spec_from_file_location('ref_ema', os.path.join(MG.REF, 'lib', 'model', 'ema.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ExponentialMovingAverage


def main():
    EMA = reference_class()
    g = torch.Generator().manual_seed(20)
    scales = 10.0 ** np.linspace(-2.0, 2.0, len(EF.SIZES))                      # magnitudes from 1e-2 to 1e2, one per tensor
    draw = lambda: [(torch.randn(n, generator=g) * float(s)).float() for n, s in zip(EF.SIZES, scales)]
    init = draw()
    params = [draw() for _ in range(EF.UPDATES)]
    params[PLANT_UPDATE - 1][PLANT_TENSOR][INF_AT] = float('inf')
    params[PLANT_UPDATE - 1][PLANT_TENSOR][NAN_AT] = float('nan')
    out = dict(sizes=np.array(EF.SIZES, np.int64), kept=np.array(EF.KEPT, np.int64), decays=np.array(EF.DECAYS, np.float64),
               init=np.concatenate([t.numpy() for t in init]), params=np.stack([np.concatenate([t.numpy() for t in ps]) for ps in params]),
               planted=np.array([PLANT_UPDATE, PLANT_TENSOR, INF_AT, NAN_AT], np.int64))
    for decay in EF.DECAYS:
        live = [torch.nn.Parameter(t.clone()) for t in init]
        ema = EMA(live, decay)
        assert all(torch.equal(s, p) and s.data_ptr() != p.data_ptr() for s, p in zip(ema.shadow_params, live))       # shadows start as clones
        mine, count, omds, kept = [t.numpy().copy() for t in init], 0, [], []
        for u in range(1, EF.UPDATES + 1):
            with torch.no_grad():
                for p, new in zip(live, params[u - 1]):
                    p.copy_(new)
            ema.update(live)
            omd, count = EF.one_minus_decay(decay, count)
            omds.append(omd)
            mine = [EF.update(s, p.numpy(), omd) for s, p in zip(mine, params[u - 1])]
            assert ema.num_updates == count == u
            for i, (s, m) in enumerate(zip(ema.shadow_params, mine)):                      # the class IS the three-rounding formula
                assert EF.same_bits(s.numpy(), m), (decay, u, i)
            if u in EF.KEPT:
                kept.append(np.concatenate([s.numpy().copy() for s in ema.shadow_params]))
        switched = [u for u in range(1, EF.UPDATES + 1) if (1 + u) / (10 + u) >= decay]        # 9 / 18 at update 8: the two meet
        assert switched == ([] if decay == 0.999 else list(range(8, EF.UPDATES + 1))), switched       # where min() takes `decay`
        sd = ema.state_dict()
        assert sd['decay'] == decay and sd['num_updates'] == EF.UPDATES and len(sd['shadow_params']) == len(EF.SIZES)
        out[f'shadow_{decay}'] = np.stack(kept)
        out[f'omd_{decay}'] = np.array(omds, np.float64)
        out['state_dict_keys'] = np.array(list(sd))
    # the contraction the kernel must not make is visible on this data: fma(-omd32, d, s) differs from the fixture somewhere
    s, omd = out['init'].astype(np.float64), float(np.float32(out['omd_0.999'][0]))
    fused = (s - omd * (out['init'] - out['params'][0]).astype(np.float32).astype(np.float64)).astype(np.float32)
    differ = int((EF.bits(fused) != EF.bits(out['shadow_0.999'][0])).sum())
    assert differ > 0, 'the fixture cannot tell a contracted multiply-subtract from the three roundings'
    path = os.path.join(HERE, 'golden_ema.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes;', differ, 'of', out['init'].size, 'elements would differ under contraction at update 1')
    assert os.path.getsize(path) < 1000000


if __name__ == '__main__':
    main()
