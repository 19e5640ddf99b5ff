"""The frozen ConvNeXt layers of a HIP training step in bf16x3 / bf16 (pipnet.set_hip_train_dtype) on the GPU.

* bf16x3 is held to the bars the fp32 step has: the stochastic-depth forward against the oracle (the case of
  test_train_forward_stochastic_depth_matches_oracle, drops forced in every block), the finetune fixtures through
  the observer forward and hip_finetune_step (test_finetune_iterations_match_reference's bars), one CountPIPNet
  finetune fixture (test_count_finetune_iterations_match_reference's bars);
* bf16 is held to the bounds tests/test_train_lowp_cpu.py measures from the reference alone and commits (cases,
  images, masks and the oracle's outputs are imported from there, computed once);
* both: a sample's rows do not depend on the batch; the step's statistics are the loss kernel's on the observer
  forward's outputs; in the joint phase the suffix and head gradients equal torch autograd through the same suffix
  modules fed the HIP frozen-prefix output (2e-3 of max |grad|, test_suffix_gradients_match_autograd's bar);
* the switch touches nothing else: set_hip_dtype alone leaves the training forward's bits, fp32 -> bf16 -> fp32
  restores them, and a step with nothing frozen (start == 0) is bitwise the fp32 step.

Measured on an MI355X (each test prints its figures): bf16x3 against the oracle on the forced-drop C2 forward pooled
2.3e-5, logits 3.3e-6 of scale; bf16 pooled 0.0101 (bound 0.027) / 0.0063 (0.017) and logits 0.086 % (0.44 %) / 0.16 %
(0.55 %) of scale on finetune_c2 / finetune_mid_addon, soft count map 0.0076 (0.021), raw counts 0.038 (0.105); joint
loss terms with a bf16 prefix within 1.2e-4 of the fp32 record, gradients within 2.3e-6 of max |grad| of autograd.
"""
import pytest
import torch

import test_train_lowp_cpu as budget
from count_pipnet_amd import kernels as K
from count_pipnet_amd import train as T
from count_pipnet_amd.convnext_features import convnext_features_hip
from count_pipnet_amd.pipnet import set_hip_dtype, set_hip_train_dtype
from golden_util import load_train_golden, train_loader_batches
from model_util import build_model
from oracle import train_ref
from test_gpu_train import _moment_close, _note_lrs, _ref_grads, _t, _trajectory_close
from train_trace_cases import (_count_setup, _finetune_setup, _optimizers_like_reference, _sd_keep, prepare,
                               record_calls, state_digest)

pytestmark = pytest.mark.gpu
LOWP = ("bf16x3", "bf16")
ROWSCALE_ENTRY = {"bf16x3": "pipnet_linear_s3_rowscale", "bf16": "pipnet_linear_bf16_mix_rowscale",
                  "fp32": "pipnet_linear_rowscale_f32"}


def _case_net(case, gpu, dtype):
    fwd_meta = budget.pipnet_case(case)[0]
    return set_hip_train_dtype(build_model(fwd_meta).to(gpu).train(), dtype)


# ---- forwards ---------------------------------------------------------------------------------------
def test_bf16x3_train_forward_stochastic_depth_matches_oracle(gpu):
    """test_train_forward_stochastic_depth_matches_oracle's model, images and tolerances, with at least one dropped
    and one kept sample in every block with p > 0, the frozen backbone in bf16x3."""
    fwd_meta, xs, ys, masks, sd, cfg, mult, (rp, rpool, rout), _ = budget.pipnet_case("finetune_c2")
    net = _case_net("finetune_c2", gpu, "bf16x3")
    with record_calls() as calls:
        proto, pooled, out = T.train_forward_hip(net, xs.to(gpu), masks)
    names = [c[0] for c in calls]
    assert names.count("pipnet_linear_s3_rowscale") == len(masks) == 17 and "pipnet_linear_rowscale_f32" not in names
    print("bf16x3 vs oracle:", budget.compare_train((proto.permute(0, 3, 1, 2), pooled, out), (rp, rpool, rout), ys,
                                                     mult, {}, check=False))
    torch.testing.assert_close(pooled.cpu(), rpool, rtol=1e-3, atol=2e-4)
    torch.testing.assert_close(out.cpu(), rout, rtol=1e-3, atol=2e-3)
    torch.testing.assert_close(proto.cpu().permute(0, 3, 1, 2), rp, rtol=1e-3, atol=2e-4)


@pytest.mark.parametrize("case", ["finetune_c2", "finetune_mid_addon"])
def test_bf16_train_forward_within_the_committed_budget(gpu, case):
    fwd_meta, xs, ys, masks, sd, cfg, mult, ref, _ = budget.pipnet_case(case)
    net = _case_net(case, gpu, "bf16")
    with record_calls() as calls:
        proto, pooled, out = T.train_forward_hip(net, xs.to(gpu), masks)
    names = [c[0] for c in calls]
    assert names.count("pipnet_linear_bf16_mix_rowscale") == len(masks) and "pipnet_linear_rowscale_f32" not in names
    got = (proto.permute(0, 3, 1, 2), pooled, out)
    print(f"bf16 vs oracle, {case}:", budget.compare_train(got, ref, ys, mult, {}, check=False))
    budget.compare_train(got, ref, ys, mult, budget.BOUNDS[case])


def _count_forward(gpu, dtype):
    fwd_meta, xs, masks, sd, cfg, noise, ref = budget.count_case()
    net = set_hip_train_dtype(build_model(fwd_meta).to(gpu).train(), dtype)
    list(net._add_on)[-1].exp_noise = noise.to(gpu)
    with torch.no_grad():
        proto, counts, _, _, _, _ = T._count_train_forward(net, xs.to(gpu), masks)
    return proto.permute(0, 3, 1, 2).cpu(), counts.cpu(), ref


def test_bf16_count_train_forward_within_the_committed_budget(gpu):
    proto, counts, (r_proto, r_counts) = _count_forward(gpu, "bf16")
    fig = dict(proto=(proto - r_proto).abs().max().item(), counts=(counts - r_counts).abs().max().item())
    print("bf16 vs oracle, count_finetune_onehot:", fig)
    assert fig["proto"] <= budget.COUNT_BOUNDS["proto"] and fig["counts"] <= budget.COUNT_BOUNDS["counts"], fig


def test_bf16x3_count_train_forward_matches_oracle(gpu):
    """The same forced-drop forward in bf16x3 at test_count_finetune_iterations_match_reference's bars."""
    proto, counts, (r_proto, r_counts) = _count_forward(gpu, "bf16x3")
    torch.testing.assert_close(proto, r_proto, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(counts, r_counts, rtol=1e-4, atol=1e-3)


# ---- finetune fixtures, bf16x3 at the fp32 bars -------------------------------------------------------
@pytest.mark.parametrize("name", ["train_finetune_mid_addon", "train_finetune_c2"])
def test_bf16x3_finetune_iterations_match_reference(gpu, name):
    meta, rec, fwd_meta, net, opt, sched, batches = _finetune_setup(name, gpu)
    set_hip_train_dtype(net, "bf16x3")
    assert T.hip_finetune_supported(net)
    cls, iters, lr_max = net._classification, len(batches), meta["lr"]
    for i, (xs1, xs2, ys) in enumerate(batches):
        sd_keep = _sd_keep(net, rec[f"s{i}_masks"])
        proto, pooled, out = T.train_forward_hip(net, torch.cat([xs1, xs2]).to(gpu), sd_keep, update_bn_stats=False)
        torch.testing.assert_close(pooled.cpu(), _t(rec[f"s{i}_pooled"]), rtol=1e-3, atol=2e-4)
        torch.testing.assert_close(out.cpu(), _t(rec[f"s{i}_out"]), rtol=1e-3, atol=2e-3)
        opt.zero_grad(set_to_none=True)
        with record_calls() as calls:
            stats = T.hip_finetune_step(net, xs1.to(gpu), xs2.to(gpu), ys.to(gpu), opt, True, sd_keep=sd_keep).cpu()
        names = [c[0] for c in calls]
        assert "pipnet_conv2d_nhwc_s3" in names and "pipnet_linear_rowscale_f32" not in names
        assert "pipnet_cnblock_mlp_hw_f32" not in names and "pipnet_dwconv7_ln_f32" not in names
        comp = meta["components"][i]
        assert float(stats[2]) == pytest.approx(comp["class"], rel=1e-3, abs=1e-4)
        assert float(stats[1]) == pytest.approx(comp["tanh"], rel=1e-3, abs=1e-4)
        assert float(stats[0]) == pytest.approx(comp["align"], rel=1e-3, abs=1e-4)
        assert float(stats[3]) == pytest.approx(comp["loss"], rel=1e-3, abs=1e-4)
        sched.step(0 + i / iters)
    st = opt.state[cls.weight]
    assert float(st["step"]) == meta["steps"]
    gw, tally = _ref_grads(rec, "_classification.weight"), [0, 0]
    if "final_w" in rec:
        _trajectory_close(cls.weight, _t(rec["final_w"]), gw, lr_max, "final weight", tally)
        _moment_close(st["exp_avg"], _t(rec["final_w_exp_avg"]), "exp_avg")
        _moment_close(st["exp_avg_sq"], _t(rec["final_w_exp_avg_sq"]), "exp_avg_sq", rel=1e-2)
    else:
        _trajectory_close(cls.weight[:8], _t(rec["final_w_rows8"]), gw, lr_max, "final weight", tally)
        _moment_close(st["exp_avg"][:8], _t(rec["final_w_exp_avg_rows8"]), "exp_avg")
    if cls.bias is not None:
        _trajectory_close(cls.bias, _t(rec["final_b"]), _ref_grads(rec, "_classification.bias"), lr_max, "final bias",
                          tally)
    assert 3 * tally[0] >= tally[1], tally


def test_bf16x3_count_finetune_iterations_match_reference(gpu):
    from count_pipnet_amd.synthetic import synth_exponential
    meta, rec, fwd_meta, net, opt, sched, batches = _count_setup("train_count_finetune_onehot", gpu)
    set_hip_train_dtype(net, "bf16x3")
    assert T.hip_count_finetune_supported(net)
    act, iters, lr_seen = list(net._add_on)[-1], len(batches), {}
    for i, (xs1, xs2, ys) in enumerate(batches):
        sd_keep = _sd_keep(net, rec[f"s{i}_masks"])
        act.exp_noise = synth_exponential(tuple(rec[f"s{i}_proto"].shape), meta["noise_seed"] + i).to(gpu)
        with torch.no_grad():
            proto, counts, clamped, _, _, out = T._count_train_forward(net, torch.cat([xs1, xs2]).to(gpu), sd_keep)
        torch.testing.assert_close(proto.permute(0, 3, 1, 2).cpu(), _t(rec[f"s{i}_proto"]), rtol=1e-3, atol=1e-4)
        r_counts = _t(rec[f"s{i}_pooled"])
        torch.testing.assert_close(counts.cpu(), r_counts, rtol=1e-4, atol=1e-3)
        ok = ((r_counts - r_counts.floor() - 0.5).abs() > 1e-3).all(dim=1)
        torch.testing.assert_close(out.cpu()[ok], _t(rec[f"s{i}_out"])[ok], rtol=1e-3, atol=2e-3)
        opt.zero_grad(set_to_none=True)
        _note_lrs(lr_seen, opt)
        stats = T.hip_count_finetune_step(net, xs1.to(gpu), xs2.to(gpu), ys.to(gpu), opt, True, 1.0,
                                          sd_keep=sd_keep).cpu()
        comp = meta["components"][i]
        assert float(stats[2]) == pytest.approx(comp["class"], rel=1e-3, abs=1e-4)
        assert float(stats[1]) == pytest.approx(comp["tanh"], rel=1e-3, abs=1e-4)
        assert float(stats[0]) == pytest.approx(comp["align"], rel=1e-3, abs=1e-4)
        assert float(stats[3]) == pytest.approx(comp["loss"], rel=1e-3, abs=1e-4)
        sched.step(0 + i / iters)
    cls, tally = net._classification, [0, 0]
    _trajectory_close(cls.weight, _t(rec["final_w"]), _ref_grads(rec, "_classification.weight"), meta["lr"],
                      "classifier weight", tally)
    _moment_close(opt.state[cls.weight]["exp_avg"], _t(rec["final_w_exp_avg"]), "exp_avg")
    assert 3 * tally[0] >= tally[1], tally


# ---- the step's statistics, per-sample invariance -----------------------------------------------------
@pytest.mark.parametrize("dtype", LOWP)
def test_step_statistics_are_the_loss_kernels_on_the_observer_forward(gpu, dtype):
    """hip_finetune_step's statistics are bitwise K.train_loss on what train_forward_hip returns with the same
    masks: the step and the observer run one forward."""
    meta, rec, fwd_meta, net, opt, sched, batches = _finetune_setup("train_finetune_mid_addon", gpu)
    set_hip_train_dtype(net, dtype)
    xs1, xs2, ys = (t.to(gpu) for t in batches[0])
    masks = budget.forced_masks(budget.golden_args(fwd_meta), 2 * xs1.shape[0], torch.Generator().manual_seed(1))
    proto, pooled, out = T.train_forward_hip(net, torch.cat([xs1, xs2]), masks)
    want, _ = K.train_loss(proto, pooled, out, ys, net._classification.normalization_multiplier, True, 1.0,
                           *T.FINETUNE_LOSS_WEIGHTS, "finetune")
    want = want.clone()
    stats = T.hip_finetune_step(net, xs1, xs2, ys, opt, True, sd_keep=masks)
    assert torch.equal(stats.cpu(), want.cpu())


@pytest.mark.parametrize("dtype", LOWP)
def test_a_sample_alone_equals_its_rows_in_the_batch(gpu, dtype):
    fwd_meta, xs, ys, masks, sd, cfg, mult, ref, _ = budget.pipnet_case("finetune_mid_addon")
    net = _case_net("finetune_mid_addon", gpu, dtype)
    xs = xs[:6].to(gpu)
    masks = {b: m[:6] for b, m in masks.items()}
    proto, pooled, out = T.train_forward_hip(net, xs, masks)
    dropped = 0
    for i in range(6):
        own = {b: m[i:i + 1] for b, m in masks.items()}
        dropped += sum(int(not m.item()) for m in own.values())
        p1, q1, o1 = T.train_forward_hip(net, xs[i:i + 1], own)
        assert torch.equal(p1[0], proto[i]) and torch.equal(q1[0], pooled[i]) and torch.equal(o1[0], out[i]), i
    assert dropped >= 5


# ---- joint phase: frozen prefix in low precision, fp32 suffix ----------------------------------------
def _suffix_autograd_grads(net, h_nhwc, start, ys, masks_in_order, w, mult):
    """Autograd through the module's own suffix (features[start:], add-on, pool, classifier) on the torch path, fed
    the HIP frozen-prefix output; stochastic-depth masks of the suffix blocks injected in forward order, loss as
    calculate_loss (align with detached targets) -- test_gpu_train._torch_path_grads from ``start`` on."""
    from count_pipnet_amd.backend import torch_backend
    orig, it = torch.Tensor.bernoulli_, iter(masks_in_order)

    def fake(self, p=0.5, *, generator=None):
        with torch.no_grad():
            self.copy_(next(it).view(self.shape).to(self.dtype))
        return self

    torch.Tensor.bernoulli_ = fake
    try:
        with torch_backend():
            x = h_nhwc.detach().permute(0, 3, 1, 2)
            for mod in net._net.features[start:]:
                x = mod(x)
            proto = net._add_on(x)
            pooled = net._pool(proto)
            out = net._classification(pooled)
    finally:
        torch.Tensor.bernoulli_ = orig
    assert next(it, None) is None
    bh = h_nhwc.shape[0] // 2
    terms = train_ref.loss_terms(proto, pooled, out, ys, mult)
    e1, e2 = train_ref.proto_pixels(proto[:bh]), train_ref.proto_pixels(proto[bh:])
    align = (train_ref.align_loss(e1, e2.detach()) + train_ref.align_loss(e2, e1.detach())) / 2
    (w[0] * align + w[1] * terms["tanh"] + w[2] * terms["cls"]).backward()
    return {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name,dtype", [("train_joint_mid_addon", "bf16x3"), ("train_joint_mid_addon", "bf16"),
                                        ("train_joint_c2", "bf16")])
def test_joint_step_with_a_low_precision_prefix(gpu, name, dtype):
    meta, rec, fwd_meta = load_train_golden(name)
    net = set_hip_train_dtype(build_model(fwd_meta).to(gpu).train(), dtype)
    opt_net, opt_cls, _, _ = _optimizers_like_reference(net, meta, fwd_meta)
    assert T.hip_train_supported(net)
    start = T.trainable_suffix_start(net)
    case = "joint_c2" if name.endswith("_c2") else "joint_mid_addon"
    assert start == budget.CASES[case][4]
    c = fwd_meta["case"]
    xs1, xs2, ys = (t.to(gpu) for t in train_loader_batches(c["size"], c["num_classes"], 1, meta["batch_per_view"],
                                                            meta["seed"])[0])
    sd_keep = _sd_keep(net, rec["s0_masks"])
    with record_calls() as calls:
        stats = T.hip_train_step(net, xs1, xs2, ys, opt_net, opt_cls, False, 1, 1, True, sd_keep=sd_keep,
                                 step_optimizers=False).cpu()
    names = [k[0] for k in calls]
    blocks = [b for mod in net._net.features[:start] for b in (mod if hasattr(mod[0], "stochastic_depth") else [])]
    assert names.count(ROWSCALE_ENTRY[dtype]) == sum(b.stochastic_depth.p > 0 for b in blocks) > 0
    hip = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    for p in net.parameters():
        p.grad = None
    # loss terms against the fp32 reference record
    comp = meta["components"][0]
    got = dict(align=float(stats[0]), tanh=float(stats[1]), cls=float(stats[2]))
    print(f"{name} {dtype}: |loss term - record|",
          {k: abs(got[k] - comp["class" if k == "cls" else k]) for k in got})
    for k, v in got.items():
        want = comp["class" if k == "cls" else k]
        if dtype == "bf16x3":
            assert v == pytest.approx(want, rel=2e-3, abs=1e-4), k        # test_suffix_training_matches_reference's
        else:
            assert abs(v - want) <= budget.BOUNDS[case][k], (k, v, want)
    # gradients against autograd through the same suffix, from the same prefix output
    with torch.no_grad():
        h = convnext_features_hip(net._net.features[:start], torch.cat([xs1, xs2]), net._net._hip_pack, sd_keep, dtype)
    n_prefix = sum(b.stochastic_depth.p > 0 for b in blocks)
    masks = [_t(m).float().to(gpu) for m in rec["s0_masks"]][n_prefix:]
    ref = _suffix_autograd_grads(net, h, start, ys, masks, (5.0, 2.0, 2.0),
                                 float(net._classification.normalization_multiplier[0]))
    assert set(hip) == set(ref), sorted(set(hip) ^ set(ref))
    worst = 0.0
    for n in sorted(ref):
        a, b = hip[n].double(), ref[n].double()
        err = (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)
        worst = max(worst, err)
        assert err < 2e-3, f"{n}: max |hip - autograd| / max|autograd| = {err:.3g}"
    print(f"{name} {dtype}: worst gradient error {worst:.3g} of max |grad| over {len(ref)} tensors")


# ---- switch isolation --------------------------------------------------------------------------------
def test_the_inference_switch_leaves_the_training_forward_alone_and_the_train_switch_restores(gpu):
    fwd_meta, xs, ys, masks, sd, cfg, mult, ref, _ = budget.pipnet_case("finetune_mid_addon")
    net = build_model(fwd_meta).to(gpu).train()
    xs = xs.to(gpu)
    base = [t.clone() for t in T.train_forward_hip(net, xs, masks)]
    set_hip_dtype(net, "bf16")
    assert all(torch.equal(a, b) for a, b in zip(T.train_forward_hip(net, xs, masks), base))
    set_hip_dtype(net, "fp32")
    for dtype in LOWP:
        set_hip_train_dtype(net, dtype)
        low = T.train_forward_hip(net, xs, masks)
        assert not torch.equal(low[2], base[2])                # the switch does reach the forward
        set_hip_train_dtype(net, "fp32")
        with record_calls() as calls:
            again = T.train_forward_hip(net, xs, masks)
        assert all(torch.equal(a, b) for a, b in zip(again, base))
        assert not [c[0] for c in calls if "s3" in c[0] or "bf16" in c[0]]


@pytest.mark.parametrize("dtype", LOWP)
def test_a_step_with_nothing_frozen_is_bitwise_the_fp32_step(gpu, dtype):
    """train_full_mid_addon trains the stem too (start == 0): no layer is frozen, so the switch changes no launch
    and no bit of the parameters and the AdamW state after one iteration."""
    digests, traces = [], []
    for d in ("fp32", dtype):
        net, opts, run = prepare("train_full_mid_addon", gpu)
        set_hip_train_dtype(net, d)
        assert T.trainable_suffix_start(net) == 0
        with record_calls() as calls:
            run(0)
        torch.cuda.synchronize()
        digests.append(state_digest(net, opts))
        traces.append(calls)
    assert traces[0] == traces[1] and digests[0] == digests[1]
