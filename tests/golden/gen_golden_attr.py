"""Generate the attribution fixtures under tests/golden/attr/ by running the REFERENCE itself.

Runs only where the reference checkout exists (as gen_golden.py).  It builds the reference models
of ``gen_golden.build_reference`` and runs the reference's own ``util/saliency_methods.IG`` / ``IDG``
behind the wrappers and the method table of ``util/interpret_idg.py`` (``PIPNetWrapper``,
``PIPNetPrototypeWrapper``, ``ATTR_FUNC``) on CPU.  interpret_idg.py cannot be imported as a module
here (it imports plotting packages and looks for its checkout's directory name at import time), so
those three definitions are compiled from its source file at run time; nothing of the reference is
written to this tree.

Per case: one image, steps 8, batch size 4, baseline 0.0, 2 prototype and 2 class targets, the three
methods each.  Per map the fixture holds

  * ``ref64``: the reference run in float64 (net, input and injected noise cast; default dtype
    float64 so that the path, the gradient store and the schedule are float64 too), stored float32;
  * ``ref_err`` = max|R32 - R64| / max|R64| of the reference's own float32 run -- what float32
    itself costs on this computation, the yardstick of the tests;
  * of the float32 run: the scores and alphas of the gradient pass, the substeps, the LeftIG cutoff,
    and for idg the first pass's slopes and step size.

Decisiveness.  A target is recorded only when nothing in its run hangs on a near-tie that another
summation order could flip (the generator moves on to the next candidate target, then to the next
noise seed, then to the next synthetic image): the LeftIG margin min_i |s_i - 0.9 max s| >= 1e-3 |max s|; every non-zero IDG placement
>= 1e-3 away from an integer; the leftover steps land on pairwise distinct positive values with gaps
>= 1e-3; a non-zero slope range; for max-pooling nets the top-two pixel gap of every prototype the
target's gradient flows through >= 1e-4 at every step; for Gumbel nets the top-two gap of the
perturbed logits >= 1e-3 at every pixel and step.

Usage:  python tests/golden/gen_golden_attr.py [--only NAME]
"""
from __future__ import annotations

import argparse
import ast
import contextlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden  # noqa: E402
from gen_golden import REF, build_reference, injected_exponential  # noqa: E402
from count_pipnet_amd.synthetic import synth_images  # noqa: E402

OUT = os.path.join(HERE, "attr")
STEPS, BATCH, BASELINE = 8, 4, 0.0
METHODS = ("ig", "lig", "idg")
SEARCH_ORDER = ("idg", "lig", "ig")      # the method most often indecisive first
N_TARGETS = 2                      # per kind
NOISE_SEEDS = 6
IMAGES = 64                        # synthetic images the search may move through
CANDIDATES = 16

# the forward cases of gen_golden.py the attribution fixtures reuse, and one of their own: the full
# ConvNeXt-tiny-26 PIP-Net (both stride-1 downsamples, stage 3 / 4 input gradients) on a 6 x 6 map
ATTR_CASES = ["pipnet_mid_addon", "count_onehot", "c1_count_identity", "count_linear_full", "pipnet_convnext26_64"]
gen_golden.CASES["pipnet_convnext26_64"] = dict(model="pipnet", net="convnext_tiny_26", num_features=0, bias=False,
                                                num_classes=10, batch=1, size=64, seed=25)


def _reference_attr():
    """(saliency_methods module, {PIPNetWrapper, PIPNetPrototypeWrapper, ATTR_FUNC}) of the reference."""
    gen_golden._import_reference()
    import util.saliency_methods as sm
    with open(os.path.join(REF, "util", "interpret_idg.py")) as f:
        lines = f.read().splitlines()
    want = {"PIPNetWrapper", "PIPNetPrototypeWrapper", "ATTR_FUNC"}
    body = []
    for i, line in enumerate(lines):       # each top-level definition on its own: the rest of the file
        head = line.split("(")[0].split(":")[0].split()          # need not parse under this interpreter
        if len(head) == 2 and head[0] in ("def", "class") and head[1] in want and not line[0].isspace():
            j = i + 1
            while j < len(lines) and (not lines[j].strip() or lines[j][0].isspace()):
                j += 1
            body += ast.parse("\n".join(lines[i:j])).body
    assert {n.name for n in body} == want
    ns = {"torch": torch, "nn": torch.nn, "IG": sm.IG, "IDG": sm.IDG}
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        exec(compile(ast.Module(body=body, type_ignores=[]), "interpret_idg.py", "exec"), ns)
    return sm, ns


class Recorder:
    """Records, during one reference attribution run, the scores of every gradient / prediction
    chunk, the schedule, the add-on output of every forward and the Gumbel module's input."""

    def __init__(self, sm, net):
        self.sm, self.net = sm, net
        self.grad_scores, self.pred_scores, self.sched, self.protos, self.gumbel_in = [], [], None, [], []

    def __enter__(self):
        sm = self.sm
        self.orig = (sm.getGradientsParallel, sm.getPredictionParallel, sm.getAlphaParameters)

        def grads(inputs, model, target):
            g, s = self.orig[0](inputs, model, target)
            self.grad_scores.append(s.detach().clone().reshape(-1))
            return g, s

        def preds(inputs, model, target):
            s = self.orig[1](inputs, model, target)
            self.pred_scores.append(s.detach().clone().reshape(-1))
            return s

        def sched(slopes, steps, step_size):
            a, sub = self.orig[2](slopes.clone(), steps, step_size)
            self.sched = (slopes.detach().clone(), float(step_size), a.detach().clone(), sub.detach().clone())
            return a, sub

        sm.getGradientsParallel, sm.getPredictionParallel, sm.getAlphaParameters = grads, preds, sched
        add_on = self.net._add_on
        self.hooks = [add_on.register_forward_hook(lambda mod, inp, out: self.protos.append(out.detach()))]
        act = add_on[-1]
        if type(act).__name__ == "GumbelSoftmax":
            self.hooks.append(act.register_forward_hook(lambda mod, inp, out: self.gumbel_in.append(
                (inp[0].detach(), float(mod.tau)))))
        return self

    def __exit__(self, *exc):
        sm = self.sm
        sm.getGradientsParallel, sm.getPredictionParallel, sm.getAlphaParameters = self.orig
        for h in self.hooks:
            h.remove()


def run_reference(sm, ns, net, case, x, kind, target, method, noise_seed, record=False):
    """One reference attribution: the map, and with ``record`` the Recorder and the noise draws."""
    count = case["model"] == "count_pipnet"
    fn = ns["ATTR_FUNC"](method)
    rec = Recorder(sm, net) if record else contextlib.nullcontext()
    with contextlib.redirect_stdout(open(os.devnull, "w")), injected_exponential(noise_seed) as drawn, rec:
        model = ns["PIPNetPrototypeWrapper"](net, count) if kind == "prototype" else ns["PIPNetWrapper"](net)
        out = fn(x.unsqueeze(0), model, STEPS, BATCH, BASELINE, torch.device("cpu"), target)
    assert torch.is_tensor(out) and tuple(out.shape) == tuple(x.shape), "the reference refused the arguments"
    return out.detach(), (rec if record else None), drawn


def placements(slopes: torch.Tensor):
    """The float placements, their truncation and the leftover count of getAlphaParameters."""
    norm = (slopes - slopes.min()) / (slopes.max() - slopes.min())
    norm[0] = 0
    placed = norm / norm.sum() * STEPS
    trunc = placed.to(torch.int32)
    return placed, trunc, int(STEPS - int(trunc.sum()))


def decisive(case, net, kind, target, method, rec, drawn) -> (bool, dict):
    """The decisiveness conditions of the module docstring on one recorded float32 run."""
    info = {}
    scores = torch.cat(rec.grad_scores)
    if method == "lig":
        mx = float(scores.max())
        info["lig_margin"] = float((scores - 0.9 * scores.max()).abs().min()) / max(abs(mx), 1e-30)
        if not (mx > 0 and info["lig_margin"] >= 1e-3):
            return False, info
    if method == "idg":
        slopes = rec.sched[0]
        if not float(slopes.max() - slopes.min()) > 0:
            return False, info
        placed, trunc, left = placements(slopes.clone())
        nz = placed[placed != 0]
        info["placement_dist"] = float((nz - nz.round()).abs().min())
        if info["placement_dist"] < 1e-3:
            return False, info
        if left > 0:
            rest = torch.sort(placed[trunc == 0], descending=True).values
            info["leftover"] = [left] + [round(float(v), 4) for v in rest[:left + 1]]
            if rest.numel() < left or float(rest[left - 1]) <= 0:
                return False, info
            top = rest[:left + 1] if rest.numel() > left else torch.cat([rest[:left], torch.zeros(1)])
            info["leftover_gap"] = float((top[:-1] - top[1:]).min())
            if info["leftover_gap"] < 1e-3 or float(rest[left - 1]) < 1e-3:
                return False, info
    count = case["model"] == "count_pipnet"
    if rec.gumbel_in:
        gap = 1e30
        for (z, tau), e in zip(rec.gumbel_in, drawn):
            g = (z - e.to(z.dtype).log()) / tau
            top = g.topk(2, dim=1).values
            gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
        info["gumbel_gap"] = gap
        if gap < 1e-3:
            return False, info
    elif not count:                  # softmax + max-pool: the argmax pixel of every prototype the gradient uses
        if kind == "prototype":
            used = torch.zeros(net._num_prototypes, dtype=torch.bool)
            used[target] = True
        else:
            used = torch.relu(net._classification.weight[target]) > 0
        gap = 1e30
        for proto in rec.protos:
            top = proto.flatten(2)[:, used].topk(2, dim=2).values
            gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
        info["pixel_gap"] = gap
        if gap < 1e-4:
            return False, info
    return True, info


def lig_cutoff(scores: torch.Tensor) -> int:
    above = torch.where(scores > scores.max() * 0.9)[0]
    cut = int(above[0]) if len(above) else 1
    return max(cut, 1)


def candidates(net, case, x, kind, noise_seed):
    """Targets ordered by their value on the image itself, largest first."""
    with torch.no_grad(), injected_exponential(noise_seed):
        _, pooled, out = net(x.unsqueeze(0), inference=False) if case["model"] == "count_pipnet" else net(x.unsqueeze(0))
    v = pooled[0] if kind == "prototype" else out[0]
    return [int(i) for i in torch.argsort(v, descending=True, stable=True)[:CANDIDATES]]


# The class targets of the full backbone's 768-prototype head cannot be decisive: a class logit's
# gradient flows through every prototype with a positive weight, and among hundreds of softmax maps
# over 768 channels some top-two pixel gap is always far below 1e-4 (1e-8 .. 3e-7 over 64 images x
# 10 classes).  That fixture records prototype targets only.
KINDS_OF = {"pipnet_convnext26_64": ("prototype",)}


def pick_targets(sm, ns, net, case, x, kinds=("prototype", "class")):
    gumbel = type(net._add_on[-1]).__name__ == "GumbelSoftmax"
    for k in range(NOISE_SEEDS if gumbel else 1):        # without Gumbel noise the seed changes nothing
        noise_seed = 2000 + 10 * case["seed"] + k
        chosen, runs = {}, {}
        for kind in kinds:
            chosen[kind] = []
            for t in candidates(net, case, x, kind, noise_seed):
                ok, kept = True, {}
                for method in SEARCH_ORDER:
                    m32, rec, drawn = run_reference(sm, ns, net, case, x, kind, t, method, noise_seed, record=True)
                    ok, info = decisive(case, net, kind, t, method, rec, drawn)
                    if not ok or not float(m32.abs().max()) > 0:
                        if os.environ.get("ATTR_GEN_VERBOSE"):
                            print(f"  seed {noise_seed} {kind} {t} {method}: rejected {info}", flush=True)
                        ok = False
                        break
                    kept[method] = (m32, rec, info, len(drawn), tuple(drawn[0].shape) if drawn else None)
                if ok:
                    chosen[kind].append(t)
                    runs[(kind, t)] = kept
                if len(chosen[kind]) == N_TARGETS:
                    break
        if all(len(v) == N_TARGETS for v in chosen.values()):
            return noise_seed, chosen, runs
    return None


def run_case(name: str) -> dict:
    sm, ns = _reference_attr()
    torch.set_default_dtype(torch.float32)
    net, case = build_reference(name)
    for k in range(IMAGES):            # the case's own image first, then further synthetic images
        image_seed = case["seed"] + 1000 * k
        x = synth_images(1, case["size"], seed=image_seed)[0]
        found = pick_targets(sm, ns, net, case, x, KINDS_OF.get(name, ("prototype", "class")))
        if found is not None:
            break
    else:
        raise RuntimeError(f"no decisive targets found for {name}")
    noise_seed, chosen, runs = found
    rec = {}
    margins = {}
    net64, _ = build_reference(name)
    net64 = net64.double()
    noise_shape, draws = None, 0
    for kind in ("prototype", "class"):
        ts = chosen.get(kind, [])
        rec[f"{kind}_targets"] = np.array(ts, dtype=np.int64)
        if not ts:
            continue
        for method in METHODS:
            maps64, errs, scores, alphas, subs, cuts, slopes, steps = [], [], [], [], [], [], [], []
            for t in ts:
                m32, r, info, n_draws, shape = runs[(kind, t)][method]
                torch.set_default_dtype(torch.float64)
                try:
                    m64, _, _ = run_reference(sm, ns, net64, case, x.double(), kind, t, method, noise_seed)
                finally:
                    torch.set_default_dtype(torch.float32)
                assert m64.dtype == torch.float64
                errs.append(float((m32.double() - m64).abs().max() / m64.abs().max()))
                maps64.append(m64.float().numpy())
                s = torch.cat(r.grad_scores)
                scores.append(s.numpy())
                cuts.append(lig_cutoff(s) if method == "lig" else STEPS)
                if method == "idg":
                    slopes.append(r.sched[0].numpy())
                    steps.append(r.sched[1])
                    alphas.append(r.sched[2].numpy())
                    subs.append(r.sched[3].numpy())
                else:
                    alphas.append(torch.linspace(0, 1, STEPS).numpy())
                margins[f"{kind}.{t}.{method}"] = info
                if shape is not None:
                    noise_shape, draws = shape, max(draws, n_draws)
            key = f"{kind}_{method}"
            rec[key + "_ref64"] = np.stack(maps64).astype(np.float32)
            rec[key + "_ref_err"] = np.array(errs, dtype=np.float64)
            rec[key + "_scores"] = np.stack(scores).astype(np.float32)
            rec[key + "_alphas"] = np.stack(alphas).astype(np.float32)
            rec[key + "_cutoff"] = np.array(cuts, dtype=np.int64)
            if method == "idg":
                rec[key + "_substeps"] = np.stack(subs).astype(np.float32)
                rec[key + "_slopes"] = np.stack(slopes).astype(np.float32)
                rec[key + "_step_size"] = np.array(steps, dtype=np.float64)
    sd = net.state_dict()
    meta = dict(name=name, case=case, profile=gen_golden.PROFILE, noise_seed=noise_seed,
                noise_shape=None if noise_shape is None else list(noise_shape), noise_draws=draws,
                image_seed=image_seed, steps=STEPS, batch_size=BATCH, baseline=BASELINE, methods=list(METHODS),
                keys=[[k, list(v.shape)] for k, v in sd.items()], margins=margins,
                input_sum=float(x.double().sum()), input_abs=float(x.double().abs().sum()), torch=torch.__version__)
    rec["meta"] = np.array(json.dumps(meta))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.set_num_threads(1)         # the recorded float32 scores are compared exactly on CPU
    os.makedirs(OUT, exist_ok=True)
    for name in ATTR_CASES:
        if a.only and name != a.only:
            continue
        rec = run_case(name)
        path = os.path.join(OUT, f"{name}.npz")
        np.savez_compressed(path, **rec)
        meta = json.loads(str(rec["meta"]))
        errs = [float(rec[k].max()) for k in rec if k.endswith("_ref_err")]
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB) targets "
              f"{rec['prototype_targets'].tolist()} / {rec['class_targets'].tolist()} image seed {meta['image_seed']} noise seed {meta['noise_seed']} "
              f"ref_err {min(float(rec[k].min()) for k in rec if k.endswith('_ref_err')):.2e}..{max(errs):.2e}",
              flush=True)


if __name__ == "__main__":
    main()
