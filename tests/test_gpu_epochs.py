"""Multi-epoch SEGAN.train on the MI355X against the reference's literal loop, batch by batch
(tests/golden/tiny_epochs*.pt, oracle/make_golden.py epochs; flavours, bars and shared checks in
tests/epochs_cases.py).  What this runs through the HIP path that nothing else does: the L1 weight
decaying and clamped at 0 (a zero-scaled regression term through the fused tanh / L1 backward), a
batch size that goes 3 -> 1 -> 3 through every cache the step keeps and through the pinned z
staging with its look-ahead draw, the epoch ends (the loader reseeds from torch's global generator
between z draws), and the asynchronous end-of-epoch Saver with its rotation.

Measured on an MI355X (deterministic mode; worst element over all tensors), next to the
reference's own float32-vs-float64 gap over the same run — the bar for the weights is 5e-5:

                               MI355X vs reference    reference fp32 vs fp64
    decay_clamp  G weights          1.16e-06               7.86e-07
                 D weights          8.75e-06 (fc.0.weight) 3.54e-06
                 losses             7.63e-06 (G_l1 = 51.6 at iteration 1; bar 1.0e-03)
                 mid G square_avg   2.10e-06 max_rel       9.92e-07
                 mid D square_avg   7.49e-06 max_rel       2.07e-06
    s2_mse       G weights          4.74e-07               3.93e-07
                 D weights          1.94e-06 (fc.2.weight) 1.11e-06
                 losses             5.72e-06 (G_l1 at iteration 3)
All three tests together: 3.3 s.
"""
import pytest
import torch

import epochs_cases as E

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def deterministic():
    """Bit-reproducible kernels for every test of this file, as in tests/test_gpu_model.py."""
    from segan_pytorch_amd import ops
    old = ops.get_deterministic()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(old)


def _run(name, tmp_path, monkeypatch):
    fx = E.load_epochs()[name]
    m, rec = E.run_train(fx, tmp_path, monkeypatch, DEV)
    torch.cuda.synchronize()
    return fx, m, rec


def test_decay_clamp_epochs_match_reference(tmp_path, monkeypatch):
    """Five epochs of B = 3, 3, 1 on the tiny stride-4 net: weight 100, then 85 ... 10, clamped to 0
    at iteration 10 and held for six iterations; five saves through the max_ckpts=3 savers."""
    fx, m, rec = _run('decay_clamp', tmp_path, monkeypatch)
    E.check_run('decay_clamp', fx, m, rec, tmp_path, 'MI355X')
    # the rotation, as the reference does it (core.py:40-51 drops the oldest once MORE than
    # max_ckpts are listed): 4 is gone, 7, 10, 13 and 16 are there
    for net in ('G-Generator', 'D-Discriminator'):
        names = sorted(n for n in fx['listing'] if n.startswith('weights_EOE_' + net))
        assert names == ['weights_EOE_{}-{}.ckpt'.format(net, s) for s in (10, 13, 16, 7)]
    # the snapshot taken while epoch 4 was already being enqueued holds the state after iteration 9
    E.check_mid_checkpoint(fx, m, tmp_path, 'MI355X')
    # a zero-scaled L1 term: exactly zero and finite through iterations 10-15, G stays finite
    assert fx['l1_weights'][9:] == [0.0] * 6 and rec['losses']['G_l1'][9:] == [0.0] * 6
    assert all(torch.isfinite(v).all() for v in m.G.state_dict().values())


def test_stride2_mse_epochs_match_reference(tmp_path, monkeypatch):
    """Three epochs of B = 2, 2, 1 on the stride-2 net with --reg_loss mse_loss, the weight decaying
    by the shipped 1e-5 from the first batch on: the small-row stride-2 kernels at B = 1."""
    fx, m, rec = _run('s2_mse', tmp_path, monkeypatch)
    E.check_run('s2_mse', fx, m, rec, tmp_path, 'MI355X')


def test_decay_clamp_epochs_are_bit_reproducible(tmp_path, monkeypatch):
    """The same loop twice in one process: deterministic mode survives the batch-size changes (the
    second run starts with every cache of the first still warm)."""
    finals = []
    for k in range(2):
        path = tmp_path / 'run{}'.format(k)
        path.mkdir()
        fx, m, rec = _run('decay_clamp', path, monkeypatch)
        finals.append(({k_: v.cpu().clone() for k_, v in m.G.state_dict().items()},
                       {k_: v.cpu().clone() for k_, v in m.D.state_dict().items()}, rec['losses']))
    for a, b in zip(finals[0][:2], finals[1][:2]):
        for k_, v in a.items():
            assert torch.equal(v, b[k_]), k_
    assert finals[0][2] == finals[1][2]
