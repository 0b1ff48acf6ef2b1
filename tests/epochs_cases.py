"""The multi-epoch literal ``SEGAN.train`` fixture (tests/golden/tiny_epochs*.pt, made by
``python oracle/make_golden.py epochs`` from the real reference) and the run / checks its tests
share: tests/test_gpu_epochs.py (HIP path), tests/test_host_orchestration.py (CPU emulation of the
kernel entry points) and tests/test_oracle.py (the fp32 oracle).

Two flavours.  'decay_clamp': the tiny stride-4 net, 7 items in batches of 3 -> B = 3, 3, 1 per
epoch, five epochs; the L1 weight is 100 in epoch 1, then 85 ... 10, is clamped to 0 at
iteration 10 and stays there; five end-of-epoch saves through the max_ckpts=3 savers.  's2_mse':
the stride-2 net with --reg_loss mse_loss, 5 items in batches of 2 -> B = 2, 2, 1, three epochs,
the weight decaying by the shipped 1e-5 from the first batch on.

Bars (none of them taken from what the code under test gives):
  weights       every element of every floating tensor within STEP_TOL = 5e-5 (10 % of one RMSprop
                step) of the reference's float32 value; D's conv.bias / norm.running_mean (NOISE_KEYS:
                a mathematically zero gradient in front of BatchNorm) are the only keys left out;
                integer buffers (num_batches_tracked) exactly.  The fixture script asserts that the
                reference itself is within STEP_TOL / 4 of the same run in float64.
  losses        at iteration i: max(ACT_TOL * max(1, |v|), 4 * gaps[loss][i]), where gaps is the
                reference's own |fp32 - fp64|; G_l1 exactly 0.0 wherever the weight is 0
  square_avg    of the mid-run checkpoint: max_rel <= max(2 * GRAD_TOL, 4 * gap)
  L1 weights, batch sizes, item order, directory listing, index files, RNG marks: exactly
"""
import functools
import json
import os
import random
from types import SimpleNamespace

import numpy as np
import torch

from conftest import load_golden, max_rel

STEP_TOL = 5e-5
ACT_TOL = 2e-5
GRAD_TOL = 1e-4
NOISE_KEYS = ('conv.bias', 'norm.running_mean')
LOSS_TAGS = ('D_real', 'D_fake', 'G_adv', 'G_l1')
FLAVOURS = ('decay_clamp', 's2_mse')
MID_STEP = 10           # weights_EOE_*-10.ckpt: written after iteration 9
# the large tensors live in files of their own, the initial weights in fixtures that had them already
PARTS = ('tiny_epochs_d.pt', 'tiny_epochs_mid_d.pt', 'tiny_epochs_mid_dsq.pt', 'tiny_epochs_s2.pt')
INIT = {'decay_clamp': 'tiny_train2.pt', 's2_mse': 'tiny_s2.pt'}


@functools.lru_cache(maxsize=None)
def load_epochs():
    """{flavour: fixture}; loaded once per process, never modified by a test."""
    fx = load_golden('tiny_epochs.pt')
    for part in PARTS:
        for (name, key), v in load_golden(part).items():
            fx[name][key] = v
    for name, src in INIT.items():
        init = load_golden(src)
        fx[name]['G0'], fx[name]['D0'] = init['G0'], init['D0']
    return fx


class PairDataset(torch.utils.data.Dataset):
    """Item i is ('u<i>', clean[i], noisy[i], 0); `served` logs the indices as the loader asks."""

    def __init__(self, clean, noisy):
        self.clean, self.noisy, self.served = clean, noisy, []

    def __len__(self):
        return self.clean.size(0)

    def __getitem__(self, i):
        self.served.append(int(i))
        return 'u{}'.format(int(i)), self.clean[i], self.noisy[i], 0


class ScalarLog(object):
    """Stands in for SummaryWriter: keeps the add_scalar calls."""

    def __init__(self, *a, **k):
        self.scalars = []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))

    def add_histogram(self, *a, **k):
        pass

    def series(self, tag):
        return [v for t, v, _ in self.scalars if t == tag]


def run_train(fx, save_path, monkeypatch, device):
    """Our SEGAN.train on the fixture's dataset, loader and seeds, log_freq=1.  Returns the model
    and what was recorded on the way."""
    from segan_pytorch_amd.models import SEGAN
    from segan_pytorch_amd.models import model as model_mod
    o = dict(fx['opts'])
    o['save_path'] = str(save_path)
    m = SEGAN(SimpleNamespace(**o))
    m.G.load_state_dict(fx['G0'])
    m.D.load_state_dict(fx['D0'])
    if device != 'cpu':
        m = m.to(device)
    ds = PairDataset(fx['clean'], fx['noisy'])
    loader = torch.utils.data.DataLoader(ds, batch_size=o['batch_size'], shuffle=True, num_workers=0)
    calls, step = [], m.gan_step

    def recording_step(clean, noisy, Gopt, Dopt, criterion, l1_weight, z=None):
        calls.append((float(l1_weight), clean.size(0)))
        return step(clean, noisy, Gopt, Dopt, criterion, l1_weight, z=z)

    m.gan_step = recording_step
    monkeypatch.setattr(model_mod, 'SummaryWriter', ScalarLog)
    random.seed(fx['run_seed'])
    np.random.seed(fx['run_seed'])
    torch.manual_seed(fx['run_seed'])
    m.train(SimpleNamespace(**o), loader, torch.nn.MSELoss(), o['l1_weight'], o['l1_dec_step'],
            o['l1_dec_epoch'], 1, va_dloader=None, device=device)
    rec = {'rand4': torch.rand(4), 'random': random.random(),
           'l1_weights': [c[0] for c in calls], 'batch_sizes': [c[1] for c in calls],
           'losses': {t: m.writer.series(t) for t in LOSS_TAGS}, 'order': []}
    served = list(ds.served)
    for b in rec['batch_sizes']:
        rec['order'].append(served[:b])
        served = served[b:]
    assert not served
    return m, rec


def weight_distance(sd, want, skip=()):
    """(worst max-abs distance over the floating tensors, its key); integer buffers must be equal."""
    worst, worst_k = 0.0, None
    for k, v in want.items():
        got = sd[k].detach().cpu()
        if not torch.is_floating_point(v):
            assert torch.equal(got, v), k
            continue
        if k.endswith(tuple(skip)):
            continue
        assert torch.isfinite(got).all(), k
        e = (got.double() - v.double()).abs().max().item()
        if e >= worst:
            worst, worst_k = e, k
    return worst, worst_k


def check_run(name, fx, m, rec, save_path, what):
    """Everything the module docstring lists, for one finished run.  Prints the measured distances."""
    # ---- host logic: exact ----
    assert rec['batch_sizes'] == fx['batch_sizes']
    assert rec['order'] == fx['order']
    assert rec['l1_weights'] == fx['l1_weights']
    assert torch.equal(rec['rand4'], fx['rand4']) and rec['random'] == fx['random']
    assert sorted(os.listdir(str(save_path))) == fx['listing']
    for prefix, want in fx['index'].items():
        with open(os.path.join(str(save_path), prefix + 'checkpoints')) as f:
            assert json.load(f) == want, prefix
    # ---- the four losses of every iteration ----
    worst_loss = (0.0, None, None)
    for t in LOSS_TAGS:
        got = rec['losses'][t]
        assert len(got) == len(fx['losses'][t]), t
        for i, (a, v) in enumerate(zip(got, fx['losses'][t])):
            assert np.isfinite(a), (t, i + 1)
            bar = max(ACT_TOL * max(1.0, abs(v)), 4 * fx['gaps']['losses'][t][i])
            if abs(a - v) > worst_loss[0]:
                worst_loss = (abs(a - v), t, i + 1)
            assert abs(a - v) <= bar, '{} at iteration {}: {} vs {} (bar {:.2e})'.format(t, i + 1, a, v, bar)
    zero = [i for i, w in enumerate(fx['l1_weights']) if w == 0]
    for i in zero:
        assert rec['losses']['G_l1'][i] == 0.0 and fx['losses']['G_l1'][i] == 0.0, i + 1
    # ---- final weights, every element ----
    g, gk = weight_distance(m.G.state_dict(), fx['G_final'])
    d, dk = weight_distance(m.D.state_dict(), fx['D_final'], skip=NOISE_KEYS)
    print('{} {}: worst weight distance G {:.2e} ({}), D {:.2e} ({}); reference fp32 vs fp64 G {:.2e}, '
          'D {:.2e}; worst loss distance {:.2e} ({} at iteration {})'.format(
              what, name, g, gk, d, dk, max(fx['gaps']['G'].values()), max(fx['gaps']['D'].values()),
              *worst_loss))
    assert g <= STEP_TOL, (gk, g)
    assert d <= STEP_TOL, (dk, d)
    return g, d, worst_loss[0]


def check_mid_checkpoint(fx, m, save_path, what):
    """'decay_clamp': the end-of-epoch-3 checkpoints hold the state after iteration 9 — weights,
    RMSprop square_avg and step count — and not a later one."""
    for net, cls, final in ((m.G, 'Generator', fx['G_final']), (m.D, 'Discriminator', fx['D_final'])):
        n = cls[0]
        skip = NOISE_KEYS if n == 'D' else ()
        ck = torch.load(os.path.join(str(save_path), 'weights_EOE_{}-{}-{}.ckpt'.format(n, cls, MID_STEP)),
                        map_location='cpu', weights_only=False)
        assert set(ck.keys()) == {'step', 'state_dict', 'optimizer'} and ck['step'] == MID_STEP
        e, k = weight_distance(ck['state_dict'], fx['mid_' + n], skip=skip)
        assert e <= STEP_TOL, (n, k, e)
        # ... and it is not the state of the end of the run
        assert any(not torch.equal(ck['state_dict'][k], net.state_dict()[k].cpu()) for k in final)
        # (the reference's own two states are `ref_far` apart and each of ours is within STEP_TOL of
        # its counterpart, so by the triangle inequality ours are at least ref_far - 2 STEP_TOL apart)
        floats = {k: v for k, v in final.items() if torch.is_floating_point(v)}
        ref_far, _ = weight_distance(fx['mid_' + n], floats, skip=skip)
        far, _ = weight_distance(ck['state_dict'], {k: net.state_dict()[k].cpu() for k in floats}, skip=skip)
        assert ref_far > 4 * STEP_TOL and far >= ref_far - 2 * STEP_TOL, (n, far, ref_far)
        names = [k for k, p in net.named_parameters() if p.requires_grad]
        st = ck['optimizer']['state']
        assert len(st) == len(names) == len(fx['mid_' + n + '_sq'])
        worst = 0.0
        for i, k in enumerate(names):
            assert float(st[i]['step']) == MID_STEP - 1, k
            if k.endswith(tuple(skip)):
                continue
            e = max_rel(st[i]['square_avg'], fx['mid_' + n + '_sq'][k])
            worst = max(worst, e)
            assert e <= max(2 * GRAD_TOL, 4 * fx['gaps'][n + '_sq'][k]), (n, k, e)
        print('{} mid-run checkpoint {}: weights {:.2e}, square_avg max_rel {:.2e} (reference fp32 vs fp64 '
              '{:.2e})'.format(what, n, weight_distance(ck['state_dict'], fx['mid_' + n], skip=skip)[0], worst,
                               max(fx['gaps'][n + '_sq'].values())))


def replay_on_oracle(fx, dtype=torch.float32):
    """The recorded batches, z, phase shifts and L1 weights through oracle.gan_step, RMSprop state
    carried from step to step.  Returns the final (G, D)."""
    import segan_oracle as O
    from conftest import oracle_kwargs
    o = fx['opts']
    cast = lambda t: t.to(dtype) if torch.is_floating_point(t) else t.clone()
    G = {k: cast(v) for k, v in fx['G0'].items()}
    D = {k: cast(v) for k, v in fx['D0'].items()}
    g_sq = d_sq = None
    losses = {t: [] for t in LOSS_TAGS}
    for i, idx in enumerate(fx['order']):
        res = O.gan_step(G, D, fx['clean'][idx].unsqueeze(1).to(dtype), fx['noisy'][idx].unsqueeze(1).to(dtype),
                         fx['z'][i].to(dtype), fx['rolls'][i], o['genc_poolings'],
                         l1_weight=fx['l1_weights'][i], lr=o['g_lr'], g_sq=g_sq, d_sq=d_sq,
                         **oracle_kwargs(o))
        G, D, g_sq, d_sq = res['G'], res['D'], res['g_sq'], res['d_sq']
        for t, k in zip(LOSS_TAGS, ('d_real_loss', 'd_fake_loss', 'g_adv_loss', 'g_l1_loss')):
            losses[t].append(float(res[k]))
    return G, D, losses
