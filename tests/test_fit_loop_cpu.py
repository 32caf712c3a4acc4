"""The host side of the tri-plane FitLoop (humanliff_amd/recon_NeRF/fit.py), no GPU: the two learning-rate schedules against the
expressions of recon_NeRF/run_nerf_batch.py:281-288, the checkpoint and optimizer-state layout against a torch.optim.Adam built as in
create_nerf (:80-89), and the refusal of a CPU module."""
import copy

import pytest
import torch

from humanliff_amd.recon_NeRF import Renderer
from humanliff_amd.recon_NeRF.fit import FitAdam, FitLoop, checkpoint_dict, lr_schedule, split_parameters


@pytest.mark.parametrize("lrate,tri_lrate,decay", [(5e-4, 1e-1, 10), (5e-4, 1e-3, 250), (0.0, 5e-3, 10)])
def test_lr_schedules_are_the_reference_expressions(lrate, tri_lrate, decay):
    for step in (0, 1, 30000, 300000, 300001):
        global_step = min(step, 300000)          # `if global_step <= 300000:` - past it the values of step 300 000 stay
        decay_rate = 0.1
        decay_steps = decay * 600
        new_lrate = lrate * (decay_rate ** (global_step / decay_steps))
        decay_rate = 0.5
        decay_steps = decay * 60
        new_tri_plane_lrate = tri_lrate * (decay_rate ** (global_step / decay_steps))
        got = lr_schedule(step, lrate, tri_lrate, decay)
        assert isinstance(got[0], float) and isinstance(got[1], float)
        assert got == (new_lrate, new_tri_plane_lrate), (step, got)


def small_module():
    torch.manual_seed(0)
    return Renderer(use_canonical_space=False, num_instances=2, triplane_dim=8, triplane_ch=27, test=False)


def reference_adam(model, lrate=5e-4, tri_plane_lrate=1e-2):
    grad_vars, tri_plane_vars = [], []
    for name, params in model.named_parameters():
        if name != 'tri_planes':
            grad_vars.append(params)
        else:
            tri_plane_vars.append(params)
    return torch.optim.Adam([{'params': grad_vars, 'lr': lrate}, {'params': tri_plane_vars, 'lr': tri_plane_lrate}], betas=(0.9, 0.999))


def structure(sd):
    """An optimizer state_dict without its numbers: keys, dtypes, shapes and devices of the state, the param_groups as they are."""
    st = {i: {k: (v.dtype, tuple(v.shape), v.device.type) if torch.is_tensor(v) else type(v) for k, v in e.items()}
          for i, e in sd['state'].items()}
    return st, sd['param_groups']


def test_optimizer_state_has_torch_adams_layout():
    ref_model = small_module()
    model = copy.deepcopy(ref_model)
    ref = reference_adam(ref_model)
    for p in ref_model.parameters():
        p.grad = torch.ones_like(p)
    ref.step()
    mlp, planes = split_parameters(model)
    assert len(mlp) == 14 and planes is model.tri_planes
    assert [tuple(p.shape) for p in mlp] == [tuple(p.shape) for p in ref.param_groups[0]['params']]
    opt = FitAdam(mlp, planes, 5e-4, 1e-2)
    fresh_st, fresh_groups = structure(opt.state_dict())
    assert fresh_st == {} and fresh_groups == structure(reference_adam(copy.deepcopy(model)).state_dict())[1]
    # a stepped state: what the HIP launches fill in is allocated by the same code on any device
    opt.init_state()
    for p in mlp + [planes]:
        opt.state[p]["step"] += 1
    assert structure(opt.state_dict()) == structure(ref.state_dict())
    # and the two load each other's files
    opt.load_state_dict(ref.state_dict())
    reference_adam(copy.deepcopy(model)).load_state_dict(opt.state_dict())
    assert torch.equal(opt.state[planes]["exp_avg"], ref.state[ref_model.tri_planes]["exp_avg"])
    assert float(opt.state[mlp[3]]["step"]) == 1.0 and opt.state[mlp[3]]["step"].device.type == "cpu"


def test_checkpoint_keys_are_the_reference_ones():
    model = small_module()
    ck = checkpoint_dict(model, FitAdam(*split_parameters(model), 5e-4, 1e-2), 7)      # (what FitLoop.checkpoint() returns)
    assert list(ck) == ['global_step', 'network_fn_state_dict', 'optimizer_state_dict'] and ck['global_step'] == 7
    assert list(ck['network_fn_state_dict']) == list(model.state_dict())
    assert set(ck['optimizer_state_dict']) == {'state', 'param_groups'}
    groups = ck['optimizer_state_dict']['param_groups']
    assert [g['params'] for g in groups] == [list(range(14)), [14]] and [g['lr'] for g in groups] == [5e-4, 1e-2]


def test_fit_loop_refuses_a_cpu_module():
    with pytest.raises(RuntimeError):
        FitLoop(small_module(), [], expname=None)
    with pytest.raises(RuntimeError):
        FitLoop(torch.nn.DataParallel(small_module()), [], ft_triplane_only=True)
