"""The one surface of the two train-mode backbone modules (convnext_train, resnet_train) and the
lookup ``train._backbone`` that picks between them, on the host: no GPU, no library load.

Nets are the fixtures' own (model_util.build_model): a full ConvNeXt, a mid-layer ConvNeXt and a
ResNet-50, on the CPU, with ``requires_grad`` set as each case needs.
"""
import inspect

import pytest
import torch
import torch.nn as nn

from count_pipnet_amd import convnext_train, resnet_train
from count_pipnet_amd import train as T
from golden_util import load_golden
from model_util import build_model

SURFACE = ("supported", "units", "trainable_start", "sd_masks", "train_forward", "backward")
NETS = {"pipnet_convnext13": convnext_train, "pipnet_mid_addon": convnext_train, "pipnet_resnet50_small": resnet_train}
PREDICATES = (T.hip_finetune_supported, T.hip_count_finetune_supported, T.hip_train_supported,
              T.hip_count_train_supported)


@pytest.fixture(scope="module")
def nets():
    return {name: build_model(load_golden(name)[0]) for name in NETS}


def _freeze(net):
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def _units(module, model):
    """The backbone's units as modules, in the order ``trainable_start`` counts them."""
    return list(model.features) if module is convnext_train else [b for _, b in resnet_train._blocks(model)]


def test_both_modules_have_the_same_surface():
    for name in SURFACE:
        a = list(inspect.signature(getattr(convnext_train, name)).parameters.values())
        b = list(inspect.signature(getattr(resnet_train, name)).parameters.values())
        shared = min(len(a), len(b))
        assert shared >= 1 and [p.name for p in a[:shared]] == [p.name for p in b[:shared]], name
        # what one module has beyond the other can be left out of a call
        assert all(p.kind is p.KEYWORD_ONLY or p.default is not p.empty for p in a[shared:] + b[shared:]), name
    assert [p.name for p in inspect.signature(convnext_train.train_forward).parameters.values()][:4] == \
        ["model", "xs", "start", "sd_keep"]
    assert [p.name for p in inspect.signature(resnet_train.backward).parameters.values()] == \
        ["model", "saved", "dfeat", "param_grads"]


def test_lookup_picks_the_module(nets):
    for name, module in NETS.items():
        net = _freeze(nets[name])
        assert T._backbone(net) is module
        assert [b.supported(net._net) for b in (convnext_train, resnet_train)] == \
            [module is convnext_train, module is resnet_train]
    plain = _freeze(nets["pipnet_mid_addon"])
    stub = nn.Module()
    stub._net, stub._add_on, stub._pool, stub._classification = nn.Sequential(nn.Conv2d(3, 8, 1)), plain._add_on, \
        plain._pool, plain._classification
    assert T._backbone(stub) is None
    assert T._backbone(nn.Linear(2, 2)) is None                  # no ``_net`` at all
    assert [f(stub) for f in PREDICATES] == [False] * 4


@pytest.mark.parametrize("name", sorted(NETS))
def test_trainable_start_and_units(nets, name):
    net, module = _freeze(nets[name]), NETS[name]
    model = net._net
    units = _units(module, model)
    n = module.units(model)
    assert n == len(units) > 1
    assert module.trainable_start(model) == n == T.trainable_suffix_start(net)          # everything frozen
    for p in units[-1].parameters():
        p.requires_grad_(True)
    assert module.trainable_start(model) == n - 1 == T.trainable_suffix_start(net)      # the last unit alone
    assert T.trainable_suffix_start(nn.DataParallel(net)) == n - 1                      # through a wrapper's .module
    if module is convnext_train:
        next(model.features[0].parameters()).requires_grad_(True)
        assert module.trainable_start(model) == 0 == T.trainable_suffix_start(net)
    else:
        model.conv1.weight.requires_grad_(True)                 # the stem never trains on the HIP path
        assert not module.supported(model) and T._backbone(net) is None
    _freeze(net)


@pytest.mark.parametrize("name", sorted(NETS))
def test_sd_masks_rng_stream(nets, name):
    net, module = _freeze(nets[name]), NETS[name]
    g = torch.Generator().manual_seed(2)
    masks = module.sd_masks(net._net, 8, g)
    if module is resnet_train:
        assert masks == {}
        assert torch.equal(g.get_state(), torch.Generator().manual_seed(2).get_state())  # nothing drawn
        assert T._sd_masks(net, 8, g) == {}
        return
    want = T.stochastic_depth_masks(net._net.features, 8, torch.Generator().manual_seed(2))
    assert list(masks) == list(want)
    assert all(masks[k].dtype == torch.bool and torch.equal(masks[k], want[k]) for k in want)
    drops = [b.stochastic_depth.p > 0.0 for b in convnext_train._cnblocks(net._net.features)]
    assert list(masks) == [i for i, d in enumerate(drops) if d]
    if masks:                                                   # the draws advanced the stream
        assert not torch.equal(g.get_state(), torch.Generator().manual_seed(2).get_state())
    again = T._sd_masks(net, 8, torch.Generator().manual_seed(2))
    assert list(again) == list(want) and all(torch.equal(again[k], want[k]) for k in want)


def test_resnet_refuses_the_input_gradient_only_backward(nets):
    with pytest.raises(NotImplementedError):
        resnet_train.backward(nets["pipnet_resnet50_small"]._net, [], torch.zeros(1), param_grads=False)
