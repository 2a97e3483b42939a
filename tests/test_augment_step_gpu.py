"""The differentiable augmentation inside the step: train_step(augment=...), GraphedStep(augment=...) and train(augment=...)."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import scrabble_oracle as O
from tests import augment_refs as AR
from tests import margins
from tests import step_fixture as F

pytestmark = pytest.mark.gpu


def _step(DU, models, gan, nlg, pb, loss, augment, opts=None, sync=True):
    from scrabble_gan_amd import optimizers
    G, D, R, S = (models[n] for n in ("G", "D", "R", "S"))
    opts = opts or [optimizers.Adam(2e-4, 0.0, 0.999) for _ in range(4)]
    return DU.train_step(0, 0, 1, pb["images"].float().numpy(), pb["labels"].numpy().astype(np.int32), D, R, S, gan, opts[0], opts[1], opts[2],
                         opts[3], pb["style"].float().numpy(), pb["B"], 128, loss, 1, 0, None, 10, "",
                         fake_labels=pb["fake"].numpy().astype(np.int32), nl=nlg, verbose=False, augment=augment)


def test_identity_tables_leave_the_step_bitwise_unchanged(dev):
    """Wiring is neutral: under deterministic mode a step with identity tables equals the step with augment=None -- the 16 scalars and
    every post-update weight of all four networks."""
    from scrabble_gan_amd import data_utils as DU, net_architecture as NA, net_loss
    pb = F.make_problem(B=8, L_r=2, L_f=2)
    ident = torch.from_numpy(np.tile(np.asarray(AR.IDENTITY, np.float32), (pb["B"], 1))).to(dev)
    runs = []
    NA.configure(device=dev, seed=9, deterministic=True)
    try:
        for aug in (None, (ident, ident.clone())):
            NA._model_counter[0] = 0
            models, gan, nlg = F.load_models(NA, pb, dev)
            out = _step(DU, models, gan, nlg, pb, net_loss.hinge, aug)
            runs.append((np.array(out, np.float64), {n: m.store.flat.clone() for n, m in models.items()},
                         {n: m.store.state.clone() for n, m in models.items()}))
    finally:
        NA.configure(deterministic=False)
    (sa, wa, ta), (sb, wb, tb) = runs
    assert np.all(np.isfinite(sa)) and np.array_equal(sa, sb), (sa, sb)
    for n in ("G", "D", "R", "S"):
        assert torch.equal(wa[n], wb[n]), "%s: post-update weights differ" % n
        assert torch.equal(ta[n], tb[n]), "%s: statistics differ" % n


# ---- the reference of the augmented step: the oracle's networks and loss, augment_refs in front of D's two calls ----------------
def _oracle_step(pb, dtype, pf, pr):
    """O.train_step's data flow (hinge, no balancing) with D seeing augment_ref(x_f) and augment_ref(images); gradients by autograd.
    -> (16 scalars, {net: {name: grad}})."""
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    nets = {n: {k: cast(v.clone()) for k, v in W.items()} for n, W in pb["P"].items()}
    nl = {n: {k: cast(v) for k, v in d.items()} for n, d in pb["nl"].items()}
    leaves = {}
    for n, P in nets.items():
        for k in P:
            if O.is_trainable(k):
                P[k] = P[k].detach().clone().requires_grad_(True)
                leaves[(n, k)] = P[k]
    images, style, labels, fake = cast(pb["images"]), cast(pb["style"]), pb["labels"], pb["fake"]
    L_r, L_f = labels.shape[1], fake.shape[1]
    x_f = O.generator(style, fake, nets["G"], nl["G.style"], nl.get("G.up"), bn_stats={})
    d_f = O.discriminator(AR.augment_ref(x_f, pf), nets["D"], nl["D.fake"])
    s_f = O.discriminator(x_f, nets["S"], nl["S.fake"])
    r_f = O.recognizer(x_f, fake, 4 * L_f - 1, L_f, nets["R"], False)
    d_r = O.discriminator(AR.augment_ref(images, pr), nets["D"], nl["D.real"])
    s_my = O.discriminator(style, nets["S"], nl["S.style"])
    s_r = O.discriminator(images, nets["S"], nl["S.real"])
    r_r = O.recognizer(images, labels, 4 * L_r - 1, L_r, nets["R"], False)
    d_loss, d_lr, d_lf, g_loss, s_loss, s_a, s_b = O.hinge(d_r, d_f, s_my, s_f, s_r)
    g_bal, r_bal, alpha, r_std, g_std = O.apply_gradient_balancing(r_f, g_loss, alpha=1)
    g_final = g_loss + r_f

    def grads_of(target, net):
        names = [k for k in nets[net] if O.is_trainable(k)]
        gs = torch.autograd.grad(target.sum(), [leaves[(net, k)] for k in names], retain_graph=True, allow_unused=True)
        return {k: (g if g is not None else torch.zeros_like(leaves[(net, k)])).detach() for k, g in zip(names, gs)}

    grads = {"D": grads_of(d_loss, "D"), "G": grads_of(g_final, "G")}
    scalars = (r_f.mean().item(), r_r.mean().item(), r_bal.mean().item(), g_loss.mean().item(), g_final.mean().item(), g_bal.mean().item(),
               d_loss.mean().item(), d_lr.mean().item(), d_lf.mean().item(), g_final.mean().item(), alpha, r_std.item(), g_std.item(),
               s_loss.mean().item(), s_a.mean().item(), s_b.mean().item())
    return scalars, grads


def test_augmented_step_against_the_composed_oracle(dev):
    """Wiring is right: fixed non-identity tables (translation + contrast for the generated images, other ones for the real images);
    the step's scalars and D's and G's gradients against the reference composed above.

    The reference is evaluated under the ReLU / max-pool decisions the HIP passes took (tests/step_fixture.forced, as
    tests/test_nets_gpu.py does; every differing decision must be a near-tie), once in fp64 and once in fp32: |fp32 - fp64| per tensor
    is what fp32 arithmetic costs on this problem, and the kernels are held to the bound of test_train_step,
        max|HIP - fp64| <= max(3 err32, 1e-3 max|ref|) + 5e-5 x the network's largest gradient,  scalars 1e-4 max(1, |ref|).
    G's gradient reaches D's input only through ops.augment_bwd: without it (dx_d added to dx_s as it leaves D) the translated and
    contrast-scaled gradient lands on the wrong pixels and G's gradients miss the bound by orders of magnitude."""
    from scrabble_gan_amd import data_utils as DU, net_architecture as NA, net_loss
    from tests.test_nets_gpu import net_atol
    pb = F.make_problem(B=4, L_r=2, L_f=2, style_w=32, seed=8, logit_scale=70.0)
    B = pb["B"]
    pf = np.asarray([AR.row(c=0.6 + 0.2 * b, beta=0.1 * b - 0.2, m=(1, 0, 3 - 2 * b, 0, 1, b - 1)) for b in range(B)], np.float32)
    pr = np.asarray([AR.row(c=1.4 - 0.2 * b, beta=0.15 - 0.1 * b, m=(1, 0, b - 2, 0, 1, 2 - b), cut=(4 * b, 8, 4 * b + 16, 24)) for b in range(B)],
                    np.float32)
    from scrabble_gan_amd.augment import DiffAugment
    DiffAugment.check(np.concatenate([pf, pr]))
    NA.configure(device=dev, seed=3)
    NA._model_counter[0] = 0
    models, gan, nlg = F.load_models(NA, pb, dev)
    DU.DEBUG_KEEP = keep = {}
    try:
        out = _step(DU, models, gan, nlg, pb, net_loss.hinge, (torch.from_numpy(pf).to(dev), torch.from_numpy(pr).to(dev)))
    finally:
        DU.DEBUG_KEEP = None
    hip_relu, hip_pool = F.hip_decisions(keep)
    del keep
    relu, pool = [hip_relu[i] for i in range(len(hip_relu))], [hip_pool[i] for i in range(len(hip_pool))]
    (s64, g64), rep = F.forced(lambda: _oracle_step(pb, torch.float64, pf, pr), relu, pool)
    F.assert_near_ties(rep, "augmented step")
    (s32, g32), _ = F.forced(lambda: _oracle_step(pb, torch.float32, pf, pr), relu, pool)
    assert len(out) == 16
    for i, (a, b) in enumerate(zip(out, s64)):
        print("scalar %2d  hip %.7e  fp64 %.7e  oracle fp32 off by %.1e" % (i, a, b, abs(s32[i] - b)))
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), "scalar %d: %r vs %r" % (i, a, b)
    bad = []
    for net in ("D", "G"):
        at = net_atol(list(g64[net].values()))
        for k, v in g64[net].items():
            scale = v.abs().max().item()
            err = (models[net].store.g[k].detach().double().cpu() - v).abs().max().item()
            e32 = (g32[net][k].double() - v).abs().max().item()
            bound = max(3.0 * e32, 1e-3 * scale) + at
            margins.record("%s grad %s" % (net, k), err / (bound / 1e-3 + 1e-30), 1e-3)
            if not err <= bound:
                bad.append("%s grad %s: max err %.3e > bound %.3e (oracle fp32 %.3e, scale %.3e)" % (net, k, err, bound, e32, scale))
    assert not bad, "\n".join(bad)


def graph_vs_eager(dev, policy):
    """Two graph replays and two eager steps from the same state, sampler state and NonLocalBlock kernels (policy None: no
    augmentation) -> [(step, scalars graph, scalars eager, [(network, max, mean |weight difference|)])], the tables of the two replays
    and whether both samplers ended in the same state."""
    from scrabble_gan_amd import data_utils as DU, net_architecture as NA, net_loss, ops, optimizers
    from scrabble_gan_amd.augment import DiffAugment
    from scrabble_gan_amd.graph_step import GraphedStep
    # (the graph test's own problem: its Adam bar was measured on these freshly initialised networks)
    B, L = 8, 3
    images, labels, my_imgs = DU.synthetic_batch(B, L, seed=3)
    fake = np.array(DU.synthetic_random_words(10, 50, seed=3)[L - 1][:B], np.int32)
    dv = [torch.from_numpy(a).to(dev) for a in (images, labels, my_imgs, fake)]
    NA._model_counter[0] = 0
    NA.configure(device=dev, seed=4)
    G = NA.make_generator(128, (32, 160, 1), (32, 8192), None, "B3", 52, vis_model=False)
    D = NA.make_discriminator((32, 160, 1), None, "B1", vis_model=False)
    R = NA.make_recognizer((32, 160, 1), None, 53, vis_model=False)
    S = NA.make_style_promoter((32, 160, 1), None, "B1", vis_model=False)
    for m in (G, D, S):
        for k in m.store.names:
            if k.endswith(".sigma"):
                m.store.p[k].fill_(0.25)
    gan = NA.make_gan(G, D, R, S, vis_model=False)
    models = (G, D, R, S)
    opts = [optimizers.Adam(2e-4, 0.0, 0.999) for _ in range(4)]
    gs = GraphedStep(D, R, S, gan, opts, B, net_loss.hinge, 0, warmup=2,
                     augment=DiffAugment(policy, seed=5, pad=0.25) if policy else None).capture(*dv)
    torch.cuda.synchronize()
    snap = [(m.store.flat.clone(), m.store.state.clone(), tuple(t.clone() for t in o._slot(m.store.flat))) for m, o in zip(models, opts)]
    aug_state = gs.augment.state() if policy else None
    out_g, nls, tables, w_graph = [], [], [], []
    for _ in range(2):
        out_g.append(np.array(tuple(gs.step()), np.float64))
        torch.cuda.synchronize()
        nls.append({n: {k: v.clone() for k, v in d.items()} for n, d in gs.nl.items()})
        tables.append(gs._aug_dev.clone() if policy else None)
        w_graph.append([m.store.flat.clone() for m in models])
    assert all(o.iterations == 4 for o in opts)
    for m, o, (flat, state, slots) in zip(models, opts, snap):
        m.store.flat.copy_(flat)
        m.store.state.copy_(state)
        for t, sv in zip(o._slot(m.store.flat), slots):
            t.copy_(sv)
        o.iterations = 2
        o.lr_dev = None              # eager steps take lr_t from their own counter (the static buffer holds the LAST replay's value)
    ops.weights_changed()
    eager = None
    if policy:
        eager = DiffAugment(policy, seed=99, pad=0.25)
        eager.set_state(aug_state)
    res = []
    for k in range(2):
        out_e = np.array(DU.train_step(0, 0, 1, dv[0], dv[1], D, R, S, gan, opts[0], opts[1], opts[2], opts[3], dv[2], B, 128, net_loss.hinge,
                                       1, 0, None, 10, "", fake_labels=dv[3], nl=nls[k], verbose=False, augment=eager), np.float64)
        w = []
        for m, wg in zip(models, w_graph[k]):
            diff = (wg - m.store.flat).abs()
            w.append((m.name, diff.max().item(), diff.mean().item()))
        res.append((k, out_g[k], out_e, w))
    return res, tables, (eager.state() == gs.augment.state()) if policy else True


def test_graph_replays_with_augmentation_equal_eager_steps(dev):
    """GraphedStep(augment=...): the rows are drawn on the host every step and reach the replay through the static [2B,12] table.  Two
    replays against two eager steps from the same state with the same sampler state and NonLocalBlock kernels, on the graph test's
    own problem: the scalars at its bound (1e-4; 2e-2 for the std / balancing entries), the weights within its Adam bar per step
    (tests/test_train_loop_gpu.py::test_graph_captured_step_equals_eager_steps)."""
    B = 8
    res, tables, same_state = graph_vs_eager(dev, "color,translation,cutout,affine")
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(tables[0][:B], tables[0][B:])      # fresh rows per step, real != fake
    assert same_state
    tol = np.full(16, 1e-4)
    tol[[2, 5, 11, 12]] = 2e-2
    bad = []
    for k, out_g, out_e, w in res:
        assert np.all(np.isfinite(out_g))
        print("step %d scalars: largest |graph - eager| / (tol max(1, |eager|)) = %.3f" % (k, np.max(np.abs(out_g - out_e) / (tol * np.maximum(1.0, np.abs(out_e))))))
        if not np.all(np.abs(out_g - out_e) <= tol * np.maximum(1.0, np.abs(out_e))):
            bad.append("step %d scalars: %s vs %s" % (k, out_g, out_e))
        for name, mx, mean in w:
            print("step %d %s: weights graph vs eager max %.3e mean %.3e" % (k, name, mx, mean))
            # (the graph test's bar for one Adam step: a component whose gradient is ~0 may step the other way, 4 lr; once per step)
            if not (mx <= (k + 1) * 4 * 2e-4 and mean <= (k + 1) * 5e-6):
                bad.append("step %d %s: max %.3e mean %.3e" % (k, name, mx, mean))
    assert not bad, "\n".join(bad)


# ---- the loop ----------------------------------------------------------------------------------------------------------------
POLICY = "color,translation,cutout"


@pytest.fixture(scope="module")
def loop_runs(dev, tmp_path_factory):
    """train() on the synthetic data in deterministic mode from one set of weights and seeds: without the keyword, with augment="",
    with the policy for two epochs, and the same stopped after epoch 1 and resumed."""
    from scrabble_gan_amd import data_utils as DU, net_architecture as NA, net_loss, ops, optimizers
    from scrabble_gan_amd.main import synthetic_dataset
    in_dim, bs, bucket = (32, 160, 1), 4, 3
    cv = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'
    pb = F.make_problem(B=8, L_r=2, L_f=2)
    root = tmp_path_factory.mktemp("augment_loop")
    res = {}
    NA.configure(device=dev, seed=6, deterministic=True)
    try:
        NA._model_counter[0] = 0
        md, gan, _ = F.load_models(NA, pb, dev)
        models = tuple(md[n] for n in ("G", "D", "R", "S"))
        G, D, R, S = models
        snap = [(m.store.flat.clone(), m.store.state.clone()) for m in models]
        words = DU.synthetic_random_words(bucket, 20, seed=2)
        my_imgs = [DU.synthetic_batch(1, 10, in_dim, 52, seed=50 + i)[2][0] for i in range(6)]

        def run(name, epochs, fresh=True, **kw):
            if fresh:
                for m, (flat, state) in zip(models, snap):
                    m.store.flat.copy_(flat)
                    m.store.state.copy_(state)
                ops.weights_changed()
            random.seed(12)
            np.random.seed(12)
            torch.manual_seed(12)
            for i, m in enumerate((G, D, S)):
                m.nl_gen.manual_seed(77 + i)
            opts = [optimizers.Adam(2e-4, 0.0, 0.999) for _ in range(4)]
            out = root / name
            DU.train(synthetic_dataset(bs, in_dim, bucket, 52, seed=3), G, D, R, S, gan, None, str(out / "ckpt"), opts[0], opts[1], opts[2],
                     opts[3], my_imgs, [None, None], 4, bs, epochs, str(out / "model"), 128, str(out / "gen"), net_loss.hinge, 1, 0, words,
                     bucket, cv, max_batches_per_epoch=2, state_path=str(out / "state.safetensors"), **kw)
            res[name] = dict(dir=out, flat=[m.store.flat.clone() for m in models], state=[m.store.state.clone() for m in models])

        run("parent", 1)
        run("off", 1, augment="")
        run("on", 2, augment=POLICY)
        run("resumed", 1, augment=POLICY)
        run("resumed", 2, fresh=False, augment=POLICY)
    finally:
        NA.configure(deterministic=False)
    return res


def _files(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _dirs, fs in os.walk(d) for f in fs)


def test_train_with_augmentation_runs_and_writes_finite_scalars(loop_runs):
    from safetensors.torch import load_file
    on, parent = loop_runs["on"], loop_runs["parent"]
    rows = (on["dir"] / "gen" / "batch_summary.txt").read_text().strip().split("\n")
    assert len(rows) == 1 + 4
    vals = np.array([[float(v) for v in r.split(";")] for r in rows[1:]])
    assert vals.shape == (4, 16) and np.all(np.isfinite(vals))
    assert rows[1:3] != (parent["dir"] / "gen" / "batch_summary.txt").read_text().strip().split("\n")[1:3]      # D saw other images
    st = load_file(str(on["dir"] / "state.safetensors"))
    assert st["rng/augment"].dtype == torch.int64 and st["rng/augment"].numel() == 10 and "rng/random" in st
    assert all(torch.isfinite(w).all() for w in on["flat"])


def test_resumed_run_with_augmentation_ends_where_the_uninterrupted_one_does(loop_runs):
    from safetensors.torch import load_file
    on, re_ = loop_runs["on"], loop_runs["resumed"]
    for a, b in zip(on["flat"] + on["state"], re_["flat"] + re_["state"]):
        assert torch.equal(a, b)
    assert (on["dir"] / "gen" / "batch_summary.txt").read_bytes() == (re_["dir"] / "gen" / "batch_summary.txt").read_bytes()
    a, b = load_file(str(on["dir"] / "state.safetensors")), load_file(str(re_["dir"] / "state.safetensors"))
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].numpy().tobytes() == b[k].numpy().tobytes(), k      # (bytes: `rng/random.gauss` is NaN when unset)


def test_augment_off_writes_what_the_run_without_the_keyword_writes(loop_runs):
    from safetensors.torch import load_file
    parent, off = loop_runs["parent"], loop_runs["off"]
    assert _files(parent["dir"]) == _files(off["dir"])
    for f in _files(parent["dir"]):
        assert (parent["dir"] / f).read_bytes() == (off["dir"] / f).read_bytes(), f
    for a, b in zip(parent["flat"] + parent["state"], off["flat"] + off["state"]):
        assert torch.equal(a, b)
    assert not [k for k in load_file(str(off["dir"] / "state.safetensors")) if k.startswith("rng/")]       # the keys the file always had
