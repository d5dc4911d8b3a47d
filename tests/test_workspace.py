"""hip.Workspace.private: a stream capture sees no workspace buffer from before it and keeps the ones it allocates.  torch records every capture on one stream, so
the key of that stream is usually in hip.Workspace already, with a buffer from an earlier graph's pool; a captured denoising loop that used it, or that replaced
it without keeping the replacement, would point into a pool that goes back to the device once its graph is gone (torch.cuda.graph.__enter__ empties the cache)."""
import pytest
import torch


def test_private_hides_and_restores_without_a_device():
    """Plain objects stand for the buffers: the manager touches only the dict."""
    from ab_opt_amd import hip
    saved = dict(hip.Workspace._bufs)
    try:
        hip.Workspace._bufs.clear()
        a, b = object(), object()
        hip.Workspace._bufs.update({(0, 1): a, (0, 2): b})
        with hip.Workspace.private() as keep:
            assert hip.Workspace._bufs == {} and keep == []
            c, d = object(), object()
            hip.Workspace._bufs[(0, 2)] = c                          # the capture stream's key, "allocated" anew inside
            hip.Workspace._bufs[(0, 3)] = d
        assert keep == [c, d]
        assert hip.Workspace._bufs == {(0, 1): a, (0, 2): b} and hip.Workspace._bufs[(0, 2)] is b
        with pytest.raises(KeyError):                                # an exception inside restores too
            with hip.Workspace.private() as keep:
                hip.Workspace._bufs[(0, 1)] = c
                raise KeyError('x')
        assert keep == [c] and hip.Workspace._bufs[(0, 1)] is a
    finally:
        hip.Workspace._bufs.clear()
        hip.Workspace._bufs.update(saved)


@pytest.mark.gpu
def test_a_captured_loop_owns_its_slab_whatever_an_earlier_capture_left():
    """With a buffer already under the capture stream's key -- a large one, which the capture could use, and a small one, which it would have to replace --
    the captured sampling loop allocates a slab of its own inside its capture and keeps it, and the earlier buffer stays where it was, the same object."""
    from ab_opt_amd import hip
    from ab_opt_amd.utils import synth
    dev = torch.device('cuda:0')
    m = synth.build_model(10, 3, device=dev)
    batch = {k: v.to(dev) for k, v in synth.make_batch(2, synth.LAYOUT_128, seed=5, lengths=[64, 57]).items()}
    torch.cuda.graph(torch.cuda.CUDAGraph())                         # creates torch's capture stream if no capture has run yet
    key = (0, torch.cuda.graph.default_capture_stream.cuda_stream)
    saved = hip.Workspace._bufs.pop(key, None)
    try:
        for nbytes in (1 << 28, 64):
            m.diffusion.clear_graphs()
            left = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            hip.Workspace._bufs[key] = left
            m.sample(batch)                                          # eager; the second call with the same signature is captured
            traj = m.sample(batch)
            torch.cuda.synchronize()
            assert len(m.diffusion._graphs) == 1 and torch.isfinite(traj[0][1]).all()
            g = next(iter(m.diffusion._graphs.values()))
            assert hip.Workspace._bufs[key] is left, nbytes
            assert len(g.keep) >= 1 and all(b is not left and b.data_ptr() != left.data_ptr() for b in g.keep), nbytes
    finally:
        m.diffusion.clear_graphs()
        hip.Workspace._bufs.pop(key, None)
        if saved is not None:
            hip.Workspace._bufs[key] = saved
