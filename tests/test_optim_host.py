"""CPU: host-side behaviour of gridnext_amd.optim (no kernel runs here).

 * construction, parameter groups, defaults and the keys of `state_dict()['param_groups']`;
 * every refusal names what it refuses: a non-fp32 parameter, amsgrad, maximize, a sparse gradient, and `step()` on CPU
   parameters ("there is no CPU path");
 * `load_state_dict` of a `torch.optim.Adam` state: `step` becomes a 0-dim float32 tensor where the parameter lives, the
   moments are unchanged; a state dict of ours configures the torch classes.
"""
import copy

import pytest
import torch
import torch.nn as nn

from gridnext_amd import optim

torch.set_num_threads(1)

SHAPES = [(3, 4), (5,), (2, 3, 2)]


def params(seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(s, generator=g).to(dtype)) for s in SHAPES]


def test_exported_from_the_package():
    import gridnext_amd as ga
    assert ga.optim is optim
    assert issubclass(optim.Adam, torch.optim.Optimizer) and issubclass(optim.AdamW, optim.Adam)


def test_defaults_and_group_keys():
    ps = params()
    o = optim.Adam(ps)
    g, = o.state_dict()['param_groups']
    assert set(g) == {'lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'decoupled_weight_decay', 'params'}
    assert (g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']) == (1e-3, (0.9, 0.999), 1e-8, 0)
    assert g['decoupled_weight_decay'] is False and g['params'] == [0, 1, 2]
    assert o.state_dict()['state'] == {}                       # state is created by the first step()
    w = optim.AdamW(ps, lr=3e-4)
    g, = w.state_dict()['param_groups']
    assert g['weight_decay'] == 1e-2 and g['decoupled_weight_decay'] is True and g['lr'] == 3e-4


def test_groups_with_their_own_hyperparameters():
    a, b, c = params()
    o = optim.Adam([{'params': [a]}, {'params': [b, c], 'lr': 1e-2, 'weight_decay': 0.1}], lr=5e-4, betas=(0.8, 0.9))
    g0, g1 = o.param_groups
    assert g0['lr'] == 5e-4 and g1['lr'] == 1e-2 and g0['weight_decay'] == 0 and g1['weight_decay'] == 0.1
    assert g0['betas'] == g1['betas'] == (0.8, 0.9)
    o.add_param_group({'params': [nn.Parameter(torch.zeros(2))], 'eps': 1e-6})
    assert len(o.param_groups) == 3 and o.param_groups[2]['eps'] == 1e-6
    for p in (a, b, c):
        p.grad = torch.ones_like(p)
    o.zero_grad()
    assert all(p.grad is None for p in (a, b, c))


@pytest.mark.parametrize('bad', [dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)),
                                 dict(weight_decay=-0.1)])
def test_invalid_hyperparameters(bad):
    with pytest.raises(ValueError):
        optim.Adam(params(), **bad)


@pytest.mark.parametrize('cls', [optim.Adam, optim.AdamW])
def test_refuses_amsgrad_and_maximize(cls):
    with pytest.raises(NotImplementedError, match="amsgrad"):
        cls(params(), amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        cls(params(), maximize=True)
    o = cls(params())
    o.param_groups[0]['amsgrad'] = True                        # switched on behind the constructor's back
    with pytest.raises(NotImplementedError, match="amsgrad"):
        o.step()


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float64])
def test_refuses_parameters_that_are_not_fp32(dtype):
    with pytest.raises(TypeError, match="float32 parameters only.*%s" % str(dtype).replace('.', r'\.')):
        optim.Adam(params(dtype=dtype))
    o = optim.Adam(params())
    with pytest.raises(TypeError, match="float32 parameters only"):
        o.add_param_group({'params': [nn.Parameter(torch.zeros(3, dtype=dtype))]})
    assert len(o.param_groups) == 1


def test_step_on_cpu_parameters_raises():
    ps = params()
    o = optim.Adam(ps)
    o.step()                                                   # no gradients: nothing to update, nothing refused
    assert o.state_dict()['state'] == {}
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU"):
        o.step()
    assert o.state_dict()['state'] == {} and len(o.state) == 0       # the refused step left no state entry behind
    assert all(torch.equal(p, q) for p, q in zip(ps, params()))     # and nothing was touched


def test_refuses_a_sparse_gradient():
    emb = nn.Embedding(6, 3, sparse=True)
    emb(torch.tensor([1, 4])).sum().backward()
    assert emb.weight.grad.is_sparse
    o = optim.Adam(emb.parameters())
    with pytest.raises(RuntimeError, match="sparse"):
        o.step()


def test_refuses_a_tensor_learning_rate():
    with pytest.raises(TypeError, match="lr as a tensor"):
        optim.Adam(params(), lr=torch.tensor(1e-3))


def torch_adam_after(n_steps, cls=torch.optim.Adam, **kw):
    ps = params()
    t = cls(ps, lr=1e-2, **kw)
    g = torch.Generator().manual_seed(1)
    for _ in range(n_steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        t.step()
    return ps, t


def test_load_state_dict_of_torch_adam():
    tps, t = torch_adam_after(3)
    ps = params()
    o = optim.Adam(ps)
    o.load_state_dict(copy.deepcopy(t.state_dict()))
    assert o.param_groups[0]['lr'] == 1e-2
    for p, tp in zip(ps, tps):
        st, ref = o.state[p], t.state[tp]
        assert torch.is_tensor(st['step']) and st['step'].dtype == torch.float32 and st['step'].dim() == 0
        assert st['step'].device == p.device and st['step'].item() == 3.0
        assert torch.equal(st['exp_avg'], ref['exp_avg']) and torch.equal(st['exp_avg_sq'], ref['exp_avg_sq'])
        assert st['exp_avg'].abs().sum() > 0
    # a checkpoint from before torch made `step` a tensor holds Python numbers
    sd = copy.deepcopy(t.state_dict())
    for st in sd['state'].values():
        st['step'] = 3
    o.load_state_dict(sd)
    assert all(o.state[p]['step'].dtype == torch.float32 and o.state[p]['step'].item() == 3.0 for p in ps)


def test_load_state_dict_refuses_amsgrad():
    _, t = torch_adam_after(1, amsgrad=True)
    o = optim.Adam(params())
    with pytest.raises(NotImplementedError, match="amsgrad"):
        o.load_state_dict(t.state_dict())
    assert o.state_dict()['state'] == {}


def test_state_dict_configures_the_torch_classes():
    for ours, theirs in ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW)):
        o = ours(params(), lr=2e-3, weight_decay=0.05)
        t = theirs(params(), foreach=False, fused=False)
        t.load_state_dict(copy.deepcopy(o.state_dict()))
        g = t.param_groups[0]
        assert g['lr'] == 2e-3 and g['weight_decay'] == 0.05
        assert g['decoupled_weight_decay'] is (ours is optim.AdamW)
        assert g['amsgrad'] is False and g['maximize'] is False
    # and AdamW stays decoupled whatever it loads, as torch's does
    w = optim.AdamW(params())
    w.load_state_dict(copy.deepcopy(optim.Adam(params()).state_dict()))
    assert w.param_groups[0]['decoupled_weight_decay'] is True
