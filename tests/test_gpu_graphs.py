"""GraphedCall (vpho_amd/model/graphs.py): Python's cycle collector does not run while the stream captures.  A dead reference cycle that
owns device memory would otherwise be freed in the middle of a capture, whenever the collector's counters say so; torch.cuda.graph
collected on entry until torch 2.10 and no longer does."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_the_collector_is_held_off_while_the_stream_captures_and_comes_back_as_it_was():
    from vpho_amd import ops
    from vpho_amd.model.graphs import GraphedCall
    seen = []

    def fn(t):
        seen.append((gc.isenabled(), torch.cuda.is_current_stream_capturing()))
        return ops.rot6d_to_axis_angle(t['a'], 4)

    a = torch.randn(4, 24, generator=torch.Generator().manual_seed(0)).cuda()
    want = ops.rot6d_to_axis_angle(a, 4)
    assert gc.isenabled()
    call = GraphedCall(fn, a.device)
    got = call({'a': a})
    assert seen == [(True, False), (False, True)]            # the eager pass, then the capture
    assert gc.isenabled() and torch.equal(got, want)
    assert torch.equal(call({'a': a}), want) and len(seen) == 2          # a replay: fn is not run again
    gc.disable()                                             # a caller that had switched the collector off keeps it off
    try:
        other = GraphedCall(fn, a.device)
        other({'a': a})
        assert not gc.isenabled() and seen[-1] == (False, True)
    finally:
        gc.enable()
