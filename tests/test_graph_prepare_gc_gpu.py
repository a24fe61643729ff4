"""optimizer.graph_prepare(), the eager call in front of a capture, collects garbage: a torch.cuda.CUDAGraph that is unreachable
in a reference cycle is destroyed there and not by a collection that happens to run while a stream is capturing, where torch's
destructor is refused and the process aborts.  Checked on the host side only: nothing here is captured."""
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu


class _Holder:
    pass


def test_graph_prepare_destroys_garbage_graphs_before_the_capture():
    from multimodal_supernovae_amd import optim
    p = torch.zeros(8, device="cuda", requires_grad=True)
    p.grad = torch.zeros_like(p)
    opt = optim.SGD([p], lr=0.1)
    was = gc.isenabled()
    gc.disable()                                        # no collection of its own between the cycle and the call
    try:
        h = _Holder()
        h.graph, h.me = torch.cuda.CUDAGraph(), h       # never captured: an empty graph object in a cycle
        alive = weakref.ref(h)
        del h
        assert alive() is not None
        opt.graph_prepare()
        assert alive() is None
    finally:
        if was:
            gc.enable()
