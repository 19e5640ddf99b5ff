"""One training iteration per tests/golden/train_*.npz fixture, as the library sees it.

``CASES`` is every train_* fixture.  ``prepare(name, gpu)`` sets the fixture's network, optimizers and
schedulers up as the reference run did (the setup helpers below are the ones tests/test_gpu_train.py uses) and
returns ``(net, optimizers, run)``; ``run(i)`` is iteration i on the HIP step of the fixture's phase, with the
fixture's recorded stochastic-depth masks and injected Gumbel noise, so no fresh seed is drawn.
``prepare(name, gpu, sharded=True)`` runs the same iteration through ``dist_train.ShardedTraining.step`` at world 1
with the exchange path forced (one shard that is the whole batch; no process group, no collective);
``SHARDED_CASES`` are the fixtures recorded that way.

``record_calls()`` wraps ``_lib.call`` -- every kernel launch goes through it -- and keeps ``[name, args]`` per
call: an argument whose entry in ``_lib.SIGNATURES[name]`` is the pointer type is kept as 0 (null) or 1, every
other one by value (floats as ``float.hex``).  ``state_digest`` is a sha256 over every parameter, every AdamW
``step`` / ``exp_avg`` / ``exp_avg_sq`` and every BatchNorm buffer.  tests/golden/gen_train_call_trace.py records
both on the parent commit into tests/golden/train_call_trace.json (``--sharded``: the sharded step, into
tests/golden/dist_train_call_trace.json); tests/test_gpu_train_trace.py and tests/test_gpu_dist_train_trace.py
hold the tree to them.
"""
import contextlib
import hashlib

import numpy as np
import torch

from count_pipnet_amd import _lib
from count_pipnet_amd import train as T
from count_pipnet_amd.convnext_features import CNBlock
from golden_util import load_train_golden, train_golden_names, train_loader_batches
from model_util import build_model

CASES = train_golden_names()
# the sharded step's record: 8 x 8 maps; every phase, a trainable stem, the Gumbel head, a bilinear layer
SHARDED_CASES = ["train_joint_mid_addon", "train_pretrain_mid_addon", "train_finetune_mid_addon",
                 "train_full_mid_addon", "train_count_joint_onehot", "train_count_joint_bilinear",
                 "train_count_finetune_bilinear"]
ITERATIONS = 2            # the trace is iteration 0; the digest is taken after iteration 1
# (kernel name, argument position) pairs that differ between two runs of the parent and are left out
MASKED = ()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _finetune_setup(name, gpu):
    meta, rec, fwd_meta = load_train_golden(name)
    net = build_model(fwd_meta).to(gpu).train()
    for prm in net.parameters():
        prm.requires_grad = False
    for prm in net._classification.parameters():
        prm.requires_grad = True
    net._classification.normalization_multiplier.requires_grad = False
    cls = net._classification
    groups = [{"params": [cls.weight], "lr": meta["lr"], "weight_decay": meta["weight_decay"]}]
    if cls.bias is not None:
        groups.append({"params": [cls.bias], "lr": meta["lr"], "weight_decay": 0.0})
    opt = torch.optim.AdamW(groups, lr=meta["lr"], weight_decay=0.0)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=10, eta_min=0.001, T_mult=1)
    c = fwd_meta["case"]
    batches = train_loader_batches(c["size"], c["num_classes"], meta["iterations"], meta["batch_per_view"],
                                   meta["seed"])
    return meta, rec, fwd_meta, net, opt, sched, batches


def _sd_keep(net, masks):
    """Recorded masks (forward order of the blocks with p > 0) -> {block id: bool mask}."""
    if not hasattr(net._net, "features"):         # ResNet: no stochastic depth
        assert masks.shape[0] == 0
        return {}
    blocks = [m for m in net._net.features.modules() if isinstance(m, CNBlock)]
    ids = [bid for bid, b in enumerate(blocks) if b.stochastic_depth.p > 0.0]
    assert len(ids) == masks.shape[0]
    return {bid: _t(masks[j]) > 0.5 for j, bid in enumerate(ids)}


# ---- pretrain / joint phases: trainable backbone suffix + add-on (+ classifier) ------------
def _optimizers_like_reference(net, meta, fwd_meta):
    """AdamW groups of util/args.py:get_optimizer_nn (restated for the test) + the phase's
    requires_grad pattern (main.py:238-256 pretrain, 377-390 joint) + its schedulers."""
    case = fwd_meta["case"]
    train, freeze, backbone = [], [], []
    for name, prm in net._net.named_parameters():
        parts = name.split(".")
        if case["net"].startswith("resnet"):     # util/args.py:280-290
            if "layer4.2" in name:
                train.append(prm)
            elif "layer4" in name or "layer3" in name:
                freeze.append(prm)
            elif "layer2" in name:
                backbone.append(prm)
        elif case.get("use_mid_layers"):
            st = int(parts[1])
            (train if st == case["num_stages"] else freeze if st == case["num_stages"] - 1 else backbone).append(prm)
        else:
            (train if "features.7.2" in name else freeze if ("features.7" in name or "features.6" in name)
             else backbone).append(prm)
    lr_net, lr_block = meta["lr_net"], meta["lr_block"]
    opt_net = torch.optim.AdamW([{"params": backbone, "lr": lr_net, "weight_decay": 0.0},
                                 {"params": freeze, "lr": lr_block, "weight_decay": 0.0},
                                 {"params": train, "lr": lr_block, "weight_decay": 0.0},
                                 {"params": list(net._add_on.parameters()), "lr": lr_block * 10.0, "weight_decay": 0.0}],
                                lr=meta["lr"], weight_decay=0.0)
    cls = net._classification
    groups = [{"params": [cls.weight], "lr": meta["lr"], "weight_decay": meta["weight_decay"]}]
    if cls.bias is not None:
        groups.append({"params": [cls.bias], "lr": meta["lr"], "weight_decay": 0.0})
    opt_cls = torch.optim.AdamW(groups, lr=meta["lr"], weight_decay=0.0)
    for prm in net.parameters():
        prm.requires_grad = False
    for prm in train + freeze + list(net._add_on.parameters()) + (backbone if meta["phase"] == "full" else []):
        prm.requires_grad = True
    for prm in cls.parameters():
        prm.requires_grad = meta["phase"] != "pretrain"
    cls.normalization_multiplier.requires_grad = False
    sched_net = torch.optim.lr_scheduler.CosineAnnealingLR(opt_net, T_max=10, eta_min=5e-6)
    sched_cls = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt_cls, T_0=10, eta_min=0.001, T_mult=1)
    return opt_net, opt_cls, sched_net, sched_cls


# ---- CountPIPNet finetune phase: classifier + intermediate layer (main.py:333-343) -----------
def _count_setup(name, gpu):
    """The reference run's setup: finetune freeze (classifier + intermediate train), the
    classifier optimizer of util/args.py:get_optimizer_nn with train_intermediate=True
    (restated for the test), CosineAnnealingWarmRestarts as main.py:314."""
    meta, rec, fwd_meta = load_train_golden(name)
    net = build_model(fwd_meta).to(gpu).train()
    cls = net._classification
    for prm in net.parameters():
        prm.requires_grad = False
    for prm in list(cls.parameters()) + list(net._intermediate.parameters()):
        prm.requires_grad = True
    cls.normalization_multiplier.requires_grad = False
    groups = [{"params": [cls.weight], "lr": meta["lr"], "weight_decay": meta["weight_decay"]},
              {"params": [] if cls.bias is None else [cls.bias], "lr": meta["lr"], "weight_decay": 0.0},
              {"params": list(net._intermediate.parameters()), "lr": meta["lr"],
               "weight_decay": meta["weight_decay"]}]
    opt = torch.optim.AdamW(groups, lr=meta["lr"], weight_decay=0.0)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=10, eta_min=0.001, T_mult=1)
    c = fwd_meta["case"]
    batches = train_loader_batches(c["size"], c["num_classes"], meta["iterations"], meta["batch_per_view"],
                                   meta["seed"])
    return meta, rec, fwd_meta, net, opt, sched, batches


# ---- CountPIPNet pretrain / joint: backbone suffix + add-on (+ classifier + intermediate) ----
def _count_suffix_setup(name, gpu):
    meta, rec, fwd_meta = load_train_golden(name)
    net = build_model(fwd_meta).to(gpu).train()
    pmeta = dict(meta, phase=meta["phase"][len("count_"):])
    opt_net, opt_cls, sched_net, sched_cls = _optimizers_like_reference(net, pmeta, fwd_meta)
    pretrain = pmeta["phase"] == "pretrain"
    inter = list(net._intermediate.parameters())
    if inter:                    # train_intermediate=True (util/args.py:318-321); main.py:251-253, 386-388
        opt_cls.add_param_group({"params": inter, "lr": meta["lr"], "weight_decay": meta["weight_decay"]})
        for prm in inter:
            prm.requires_grad = not pretrain
        sched_cls = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt_cls, T_0=10, eta_min=0.001, T_mult=1)
    c = fwd_meta["case"]
    batches = train_loader_batches(c["size"], c["num_classes"], meta["iterations"], meta["batch_per_view"],
                                   meta["seed"])
    return meta, rec, fwd_meta, net, opt_net, opt_cls, sched_net, sched_cls, pretrain, batches


def _inject_noise(net, meta, rec, i, gpu):
    from count_pipnet_amd.count_pipnet_utils import GumbelSoftmax
    from count_pipnet_amd.synthetic import synth_exponential
    act = list(net._add_on)[-1]
    if isinstance(act, GumbelSoftmax):
        act.exp_noise = synth_exponential(tuple(rec[f"s{i}_proto"].shape), meta["noise_seed"] + i).to(gpu)


# ---- one iteration per fixture -------------------------------------------------------------
def prepare(name, gpu, sharded=False):
    """(net, optimizers, run) of a fixture; ``run(i)`` is iteration i as the fixture's test steps it, ``sharded``:
    through ``ShardedTraining(net, seed=5, force_exchange=True).step`` at world 1."""
    count, finetune = name.startswith("train_count_"), "_finetune_" in name
    if finetune:
        meta, rec, _, net, opt, sched, batches = (_count_setup if count else _finetune_setup)(name, gpu)
        opts, sched_net, sched_cls, pretrain = [opt], None, sched, False
    elif count:
        meta, rec, _, net, opt_net, opt_cls, sched_net, sched_cls, pretrain, batches = _count_suffix_setup(name, gpu)
        opts = [opt_net, opt_cls]
    else:
        meta, rec, fwd_meta = load_train_golden(name)
        net = build_model(fwd_meta).to(gpu).train()
        opt_net, opt_cls, sched_net, sched_cls = _optimizers_like_reference(net, meta, fwd_meta)
        opts, pretrain = [opt_net, opt_cls], meta["phase"] == "pretrain"
        c = fwd_meta["case"]
        batches = train_loader_batches(c["size"], c["num_classes"], meta["iterations"], meta["batch_per_view"],
                                       meta["seed"])
    assert len(batches) >= ITERATIONS, name
    st = None
    if sharded:
        from count_pipnet_amd.dist_train import ShardedTraining
        st = ShardedTraining(net, seed=5, force_exchange=True)
        assert st.world == 1 and st.process_group is None

    def run(i):
        xs1, xs2, ys = (t.to(gpu) for t in batches[i])
        sd_keep = _sd_keep(net, rec[f"s{i}_masks"])
        if count:
            _inject_noise(net, meta, rec, i, gpu)
        for opt in opts:
            opt.zero_grad(set_to_none=True)
        if sharded:
            st.step(xs1, xs2, ys, None if finetune else opts[0], opts[-1], epoch=1, nr_epochs=2 if pretrain else 1,
                    phase="finetune" if finetune else "pretrain" if pretrain else "train", sd_keep=sd_keep)
        elif finetune and count:
            T.hip_count_finetune_step(net, xs1, xs2, ys, opts[0], True, 1.0, sd_keep=sd_keep)
        elif finetune:
            T.hip_finetune_step(net, xs1, xs2, ys, opts[0], True, sd_keep=sd_keep)
        elif count:
            T.hip_count_train_step(net, xs1, xs2, ys, opts[0], opts[1], pretrain, 1, 2 if pretrain else 1, True,
                                   1.0, sd_keep=sd_keep)
        else:
            T.hip_train_step(net, xs1, xs2, ys, opts[0], opts[1], pretrain, 1, 2 if pretrain else 1, True,
                             sd_keep=sd_keep)
        if not pretrain:
            sched_cls.step(0 + i / len(batches))
        if not finetune:
            sched_net.step()

    return net, opts, run


@contextlib.contextmanager
def record_calls(masked=MASKED):
    """Within the context every ``_lib.call`` is appended to the yielded list as ``[name, args]``; a
    ``(kernel name, argument position)`` of ``masked`` is kept as None."""
    calls, real = [], _lib.call

    def recording(name, *args):
        row = []
        for pos, (kind, a) in enumerate(zip(_lib.SIGNATURES[name], args)):
            if (name, pos) in masked:
                row.append(None)
            elif kind is _lib.P:
                row.append(int(bool(a)))
            else:
                row.append(float(a).hex() if isinstance(a, float) else int(a))
        assert len(args) == len(_lib.SIGNATURES[name]), name
        calls.append([name, row])
        return real(name, *args)

    _lib.call = recording
    try:
        yield calls
    finally:
        _lib.call = real


def state_digest(net, optimizers):
    """sha256 over every parameter, every AdamW state tensor and every BatchNorm buffer (names included)."""
    h = hashlib.sha256()

    def add(key, t):
        h.update(key.encode() + b"\0" + t.detach().cpu().contiguous().numpy().tobytes() + b"\0")

    names = {id(p): n for n, p in net.named_parameters()}
    for n, p in net.named_parameters():
        add("param/" + n, p)
    for k, opt in enumerate(optimizers):
        for g in opt.param_groups:
            for p in g["params"]:
                for key in ("step", "exp_avg", "exp_avg_sq"):
                    if key in opt.state.get(p, {}):
                        add(f"opt{k}/{names[id(p)]}/{key}", opt.state[p][key])
    for mn, mod in net.named_modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            for bn, b in mod.named_buffers(recurse=False):
                add(f"buffer/{mn}.{bn}", b)
    return h.hexdigest()


def trace_and_digest(name, gpu, sharded=False):
    """Iteration 0's library calls and the state digest after ``ITERATIONS`` iterations."""
    net, opts, run = prepare(name, gpu, sharded)
    with record_calls() as calls:
        run(0)
    for i in range(1, ITERATIONS):
        run(i)
    torch.cuda.synchronize()
    return calls, state_digest(net, opts)
