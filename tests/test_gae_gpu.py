"""GPU tests of dcomp_gae (deepcomp_amd/sampler.py: gae): advantages and value_targets are BIT-identical to sampler.gae_reference --
the float32 operations of RLlib's compute_advantages(use_gae=True), each rounded on its own -- at every T x R of the grid below
(R = 63 / 64 / 65: around a wavefront; 4 099: more than one workgroup, not a multiple of anything) and every way an episode can end
inside the batch.  Inputs: rewards uniform in [-1, 1], values N(0, 1), gamma = 0.99: all magnitudes are normal float32, so denormal
handling cannot decide the comparison."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS, RS = [1, 2, 7, 50], [1, 63, 64, 65, 4099]
GAMMA = 0.99


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _ends(T):
    """name -> end flags [T] (None: the NULL pointer); cases that need more steps than T has are left out."""
    e = {'none': None, 'at_0': [0], 'at_last': [T - 1]}
    if T >= 7:
        e['two_inside'] = [2, T - 3]
    return e


@pytest.mark.parametrize('lam', [1.0, 0.95])
@pytest.mark.parametrize('R', RS)
@pytest.mark.parametrize('T', TS)
def test_gae_is_bit_identical_to_the_reference(torch_cuda, T, R, lam):
    torch = torch_cuda
    from deepcomp_amd.sampler import gae, gae_reference
    rng = np.random.default_rng(1000 * T + R)
    rew = rng.uniform(-1, 1, size=(T, R)).astype(np.float32)
    vf = rng.normal(size=(T, R)).astype(np.float32)
    last = rng.normal(size=R).astype(np.float32)
    d_rew, d_vf = torch.from_numpy(rew).cuda(), torch.from_numpy(vf).cuda()
    for name, at in _ends(T).items():
        end = None
        if at is not None:
            end = np.zeros(T, dtype=np.uint8)
            end[at] = 1
        for last_vf in (last, None):
            lv = last_vf
            if name == 'at_last' and last_vf is not None:
                lv = np.full(R, np.nan, dtype=np.float32)              # the batch ends with its episode: last_vf must not matter
            want_a, want_t = gae_reference(rew, vf, lv, end, GAMMA, lam)
            adv = torch.full((T, R), float('nan'), device='cuda')
            tgt = torch.full((T, R), float('nan'), device='cuda')
            got = gae(d_rew, d_vf, torch.from_numpy(lv).cuda() if lv is not None else None,
                      torch.from_numpy(end).cuda() if end is not None else None, GAMMA, lam, out=(adv, tgt))
            assert got[0] is adv and got[1] is tgt
            a, t = adv.cpu().numpy(), tgt.cpu().numpy()
            assert np.isfinite(a).all() and np.isfinite(t).all(), (name, last_vf is None)
            assert np.isfinite(want_a).all()
            assert np.array_equal(_bits(a), _bits(want_a)), (name, last_vf is None, int((a != want_a).sum()))
            assert np.array_equal(_bits(t), _bits(want_t)), (name, last_vf is None, int((t != want_t).sum()))


def test_gae_checks_its_tensors(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd.sampler import gae
    rew, vf = torch.zeros((3, 5), device='cuda'), torch.zeros((3, 5), device='cuda')
    a, t = gae(rew, vf)
    assert a.shape == t.shape == (3, 5) and a.dtype == torch.float32
    for kw in (dict(vf=torch.zeros((3, 4), device='cuda')), dict(vf=vf.double()), dict(vf=vf.cpu()), dict(last_vf=torch.zeros(4, device='cuda')),
               dict(end=torch.zeros(3, device='cuda')), dict(end=torch.zeros(2, dtype=torch.uint8, device='cuda')),
               dict(out=(torch.zeros((3, 5), device='cuda'), torch.zeros((2, 5), device='cuda')))):
        args = dict(reward=rew, vf=vf)
        args.update(kw)
        with pytest.raises(ValueError):
            gae(**args)
    torch.cuda.synchronize()
