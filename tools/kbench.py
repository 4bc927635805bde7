#!/usr/bin/env python3
"""Micro-benchmark of single kernels of the hot path at BASELINE config-2 shapes (GPU only).

    python tools/kbench.py [fwd|bwd|epi|dx|skip|decode|ae|guard|ema|nll|win_nll|wnll|cond|vq|vq_ema|gcond|gclass|phase|rvq|all] [--reps N] [--precision f16x3,bf16x3]

Prints per-phase / per-layer kernel times measured with HIP events on the launch stream.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CFG, B_LOCAL, T  # noqa: E402


def _median_spread(v):
    v = sorted(v)
    return round(float(np.median(v)), 3), round(v[-1] - v[0], 3)


def vq_bench(reps, alternations=6):
    """`vq`: the vector-quantised bottleneck.  (a) wn_vq_fwd and wn_vq_bwd alone at config 4's shape (B 8, Bw 64, Le 25, K 512) and at
    the shipped autoencoder's (B 4, Bw 512, Le 32, K 512), HIP events around `reps` launches; (b) the fused config-4 step (forward,
    loss, backward, flat Adam) of a vq model against the continuous model, both with learned conditioning.  Everything is
    alternated `alternations` times on one device: medians and spreads (largest - smallest) over the alternations."""
    import time
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.model1 import wavenet_autoencoder
    st = _lib.stream()
    res = {"alternations": alternations}
    rng = np.random.default_rng(0)
    shapes = {"config4": (8, 64, 25, 512), "shipped": (4, 512, 32, 512)}
    bufs = {}
    for name, (B, Bw, Le, K) in shapes.items():
        enc = torch.from_numpy(rng.standard_normal((B, Bw, Le)).astype(np.float32)).cuda()
        flat = torch.from_numpy(rng.standard_normal(K * Bw).astype(np.float32)).cuda()
        bufs[name] = dict(enc=enc, flat=flat, q=torch.empty_like(enc), idx=torch.empty(B, Le, dtype=torch.int32, device="cuda"),
                          counts=torch.empty(K, dtype=torch.int32, device="cuda"),
                          part=torch.empty(_lib.VQ_NUM_PARTIALS, dtype=torch.float32, device="cuda"), d=torch.randn_like(enc),
                          grad=torch.empty_like(flat))

    def launches(name, which, n):
        B, Bw, Le, K = shapes[name]
        b = bufs[name]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(n):
            if which == "fwd":
                call("wn_vq_fwd", ptr(b["enc"]), ptr(b["flat"]), 0, ptr(b["q"]), ptr(b["idx"]), ptr(b["counts"]), ptr(b["part"]), K, Bw, Le, B, st)
            else:
                call("wn_vq_bwd", ptr(b["enc"]), ptr(b["idx"]), ptr(b["d"]), ptr(b["flat"]), 0, 0.25, 1.0, ptr(b["d"]), ptr(b["grad"]), K, Bw,
                     Le, B, st)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n * 1e3
    times = {(n, w): [] for n in shapes for w in ("fwd", "bwd")}
    for key in times:
        launches(*key, 20)                                                    # warm
    for _ in range(alternations):
        for key in times:
            times[key].append(launches(*key, max(reps, 100)))
    for (n, w), v in times.items():
        res["wn_vq_%s_%s_us" % (w, n)], res["wn_vq_%s_%s_us_spread" % (w, n)] = _median_spread(v)
    # ---- the fused config-4 step
    cfg = dict(filter_width=2, quantization_channel=256, dilations=CFG["dilations"], en_residual_channel=64, en_dilation_channel=64,
               en_bottleneck_width=64, en_pool_kernel_size=512, de_residual_channel=64, de_dilation_channel=64, de_skip_channel=256,
               use_bias=False, conditioning="learned")
    codes = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL, T)).astype(np.int32)).cuda()
    engs = {}
    for mode in ("continuous", "vq"):
        torch.manual_seed(0)
        net = wavenet_autoencoder(bottleneck=mode, vq_codes=512, **cfg).cuda()
        eng = net._engine_for(torch.device("cuda", 0))
        eng.adam_init(lr=1e-4)
        engs[mode] = (net, eng)
    from music_amd.faster_audio_data import onehot_device
    x = onehot_device(codes, 256, True)
    W = T - engs["vq"][0].receptive_field + 1
    target = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL * W,)).astype(np.int64)).cuda()
    with torch.no_grad():
        _, _, ws0 = engs["vq"][1].forward(x, None, want_probs=False, encode_only=True)
    engs["vq"][0].init_codebook(ws0["enc_pre"], seed=0)                       # (codes in use, as in a trained model)

    def steps(mode, n):
        eng = engs[mode][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = eng.loss_and_grad(x, target, None)
            eng.adam_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(loss)
    for mode in engs:
        steps(mode, 5)
    step_ms = {m: [] for m in engs}
    for _ in range(alternations):
        for mode in engs:
            ms, loss = steps(mode, max(reps, 20))
            step_ms[mode].append(ms)
            res["fused_step_loss_" + mode] = round(loss, 5)
    for mode, v in step_ms.items():
        res["fused_step_ms_" + mode], res["fused_step_ms_%s_spread" % mode] = _median_spread(v)
    res["fused_step_ms_vq_minus_continuous"] = round(res["fused_step_ms_vq"] - res["fused_step_ms_continuous"], 3)
    res["fused_step_ms_by_alternation"] = {m: [round(t, 3) for t in v] for m, v in step_ms.items()}
    stats = engs["vq"][1].last_vq
    res["vq_codes_used"], res["vq_perplexity"] = int(stats.codes_used), round(float(stats.perplexity), 2)
    res["shape_config4_step"] = dict(B=B_LOCAL, T=T, frames=B_LOCAL * (W // 512), Bw=64, K=512)
    print(json.dumps(res))


def vq_ema_bench(reps, alternations=6):
    """`vq_ema`: EMA codebook updates.  (a) wn_vq_bwd_stats (beside wn_vq_bwd, whose place it takes) and the two launches of
    wn_vq_ema_update alone at config 4's shape (B 8, Bw 64, Le 25, K 512) and at the shipped autoencoder's (B 4, Bw 512, Le 32,
    K 512), HIP events around `reps` calls; (b) the fused config-4 step of an ema model against the gradient model, both started from
    a data-drawn codebook; everything alternated `alternations` times on one device, medians and spreads (largest - smallest);
    (c) the collapse the mode exists for: perplexity and codes in use on the bench batch from the constructor's codebook after the
    warm-up steps and after 100 more, with vq_restart off and on.  Written to profiles/vq_ema_kbench.json."""
    import time
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.model1 import wavenet_autoencoder
    st = _lib.stream()
    res = {"alternations": alternations}
    rng = np.random.default_rng(0)
    shapes = {"config4": (8, 64, 25, 512), "shipped": (4, 512, 32, 512)}
    bufs = {}
    for name, (B, Bw, Le, K) in shapes.items():
        enc = torch.from_numpy(rng.standard_normal((B, Bw, Le)).astype(np.float32)).cuda()
        flat = torch.from_numpy(rng.standard_normal(K * Bw).astype(np.float32)).cuda()
        idx = torch.from_numpy(rng.integers(0, K, size=(B, Le)).astype(np.int32)).cuda()
        bufs[name] = dict(enc=enc, flat=flat, idx=idx, d=torch.randn_like(enc), grad=torch.empty_like(flat),
                          stat=torch.zeros(K * (Bw + 1), device="cuda"), state=torch.cat([torch.ones(K, device="cuda"), flat]),
                          work=torch.zeros(_lib.VQ_EMA_WORK_BYTES // 4, dtype=torch.int32, device="cuda"),
                          info=torch.zeros(2, dtype=torch.int32, device="cuda"))

    def launches(name, which, n):
        B, Bw, Le, K = shapes[name]
        b = bufs[name]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(n):
            if which == "bwd":
                call("wn_vq_bwd", ptr(b["enc"]), ptr(b["idx"]), ptr(b["d"]), ptr(b["flat"]), 0, 0.25, 1.0, ptr(b["d"]), ptr(b["grad"]), K, Bw,
                     Le, B, st)
            elif which == "bwd_stats":
                call("wn_vq_bwd_stats", ptr(b["enc"]), ptr(b["idx"]), ptr(b["d"]), ptr(b["flat"]), 0, 0.25, 1.0, ptr(b["d"]), ptr(b["grad"]),
                     ptr(b["stat"]), K, Bw, Le, B, st)
            else:                                                               # (its two launches; restarts on: a used code's N' stays >= 1)
                call("wn_vq_ema_update", ptr(b["flat"]), 0, ptr(b["stat"]), ptr(b["state"]), ptr(b["work"]), ptr(b["info"]), K, Bw, 0.99, 1e-5,
                     0.995, None, st)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n * 1e3
    times = {(n, w): [] for n in shapes for w in ("bwd", "bwd_stats", "ema_update")}
    for key in times:
        launches(*key, 20)                                                    # warm (and the stats the update reads exist)
    for _ in range(alternations):
        for key in times:
            times[key].append(launches(*key, max(reps, 100)))
    for (n, w), v in times.items():
        res["wn_vq_%s_%s_us" % (w, n)], res["wn_vq_%s_%s_us_spread" % (w, n)] = _median_spread(v)
    # ---- the fused config-4 step
    cfg = dict(filter_width=2, quantization_channel=256, dilations=CFG["dilations"], en_residual_channel=64, en_dilation_channel=64,
               en_bottleneck_width=64, en_pool_kernel_size=512, de_residual_channel=64, de_dilation_channel=64, de_skip_channel=256,
               use_bias=False, conditioning="learned", bottleneck="vq", vq_codes=512)
    codes = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL, T)).astype(np.int32)).cuda()
    from music_amd.faster_audio_data import onehot_device
    x = onehot_device(codes, 256, True)

    def model(**kw):
        torch.manual_seed(0)
        net = wavenet_autoencoder(**dict(cfg, **kw)).cuda()
        eng = net._engine_for(torch.device("cuda", 0))
        eng.adam_init(lr=1e-4)
        return net, eng
    engs = {"gradient": model(), "ema": model(vq_update="ema", vq_restart=0.995)}
    W = T - engs["ema"][0].receptive_field + 1
    target = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL * W,)).astype(np.int64)).cuda()
    with torch.no_grad():
        _, _, ws0 = engs["ema"][1].forward(x, None, want_probs=False, encode_only=True)
    for net, _ in engs.values():
        net.init_codebook(ws0["enc_pre"], seed=0)                             # (codes in use, as in a trained model)

    def steps(eng, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = eng.loss_and_grad(x, target, None)
            eng.adam_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(loss)
    for mode in engs:
        steps(engs[mode][1], 5)
    step_ms = {m: [] for m in engs}
    for _ in range(alternations):
        for mode in engs:
            ms, loss = steps(engs[mode][1], max(reps, 20))
            step_ms[mode].append(ms)
            res["fused_step_loss_" + mode] = round(loss, 5)
    for mode, v in step_ms.items():
        res["fused_step_ms_" + mode], res["fused_step_ms_%s_spread" % mode] = _median_spread(v)
    res["fused_step_ms_ema_minus_gradient"] = round(res["fused_step_ms_ema"] - res["fused_step_ms_gradient"], 3)
    res["fused_step_ms_by_alternation"] = {m: [round(t, 3) for t in v] for m, v in step_ms.items()}
    res["ema_update_restarted_in_timed_steps"] = engs["ema"][1].vq_restarted()
    res["shape_config4_step"] = dict(B=B_LOCAL, T=T, frames=B_LOCAL * (W // 512), Bw=64, K=512)
    # ---- the collapse: the constructor's codebook on the bench batch
    for label, kw in (("gradient", {}), ("ema_restart_off", dict(vq_update="ema")), ("ema_restart_on", dict(vq_update="ema", vq_restart=0.995))):
        net, eng = model(**kw)
        for n_steps, when in ((5, "after_warmup"), (100, "after_105_steps")):
            steps(eng, n_steps)
            eng.loss_and_grad(x, target, None)
            s = eng.last_vq
            res["collapse_%s_%s" % (label, when)] = dict(codes_used=int(s.codes_used), perplexity=round(float(s.perplexity), 2))
        if eng.vq_ema:
            res["collapse_%s_restarted" % label] = eng.vq_restarted()
    print(json.dumps(res))


def _write_profile(name, res):
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def bench_unset(parent, alternations=6, profile="gcond_bench_unset.json", keys="global_classes / global_channels"):
    """bench.py of this tree (the new keys unset: the feature launches nothing there) against a built checkout of the parent commit at
    `parent`, alternated `alternations` times, each run a process of its own.  Called before this process touches the device."""
    import subprocess
    runs = {"parent": [], "tree": []}
    for _ in range(alternations):
        for label, root in (("parent", parent), ("tree", ROOT)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "60", "--warmup", "20"], cwd=root, check=True,
                                 stdout=subprocess.PIPE, timeout=300).stdout.decode()
            line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            runs[label].append({k: line[k] for k in ("ms_per_step", "value") if k in line})
    res = {"what": "bench.py --gpus 1 --steps 60 --warmup 20 with %s unset, parent commit and this tree "
                   "alternating on one MI355X, %d pairs, parent first" % (keys, alternations)}
    res.update(runs)
    for label, v in runs.items():
        ms = [r["ms_per_step"] for r in v if "ms_per_step" in r]
        if ms:
            res[label + "_ms_per_step_median"], res[label + "_ms_per_step_spread"] = _median_spread(ms)
    _write_profile(profile, res)
    print(json.dumps(res))


def rvq_bench(reps, alternations=6):
    """`rvq`: residual vector quantisation.  (a) wn_rvq_fwd / wn_rvq_bwd / wn_rvq_ema_update at S = 2, 4, 8 against the composition they
    replace, built from the one-stage entries: S wn_vq_fwd launches with the torch subtractions and additions between them, S
    wn_vq_bwd launches, S wn_vq_ema_update calls - at config 4's shape (B 8, Bw 64, Le 25, K 512) and the shipped autoencoder's
    (B 4, Bw 512, Le 32, K 512), HIP events around `reps` rounds; (b) the fused config-4 step at S = 4 against S = 1, both learned.
    Everything alternated `alternations` times on one device: medians and spreads.  Written to profiles/rvq_kbench.json."""
    import time
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.model1 import wavenet_autoencoder
    st = _lib.stream()
    res = {"alternations": alternations}
    rng = np.random.default_rng(0)
    shapes = {"config4": (8, 64, 25, 512), "shipped": (4, 512, 32, 512)}
    stages = (2, 4, 8)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device="cuda")
    bufs = {}
    for name, (B, Bw, Le, K) in shapes.items():
        for S in stages:
            enc = torch.from_numpy(rng.standard_normal((B, Bw, Le)).astype(np.float32)).cuda()
            flat = torch.from_numpy(np.concatenate([rng.standard_normal(K * Bw) * 0.8 ** s for s in range(S)]).astype(np.float32)).cuda()
            b = bufs[name, S] = dict(enc=enc, flat=flat, q=f32(B, Bw, Le), idx=i32(S, B, Le), counts=i32(S, K), res=f32(S, B, Bw, Le),
                                     part=f32(S, _lib.VQ_NUM_PARTIALS), d=torch.randn_like(enc), d_out=f32(B, Bw, Le), grad=torch.empty_like(flat),
                                     stat=f32(S, K * (Bw + 1)), state=f32(S, K * (Bw + 1)), work=i32(S, _lib.VQ_EMA_WORK_BYTES // 4), info=i32(S, 2))
            call("wn_rvq_fwd", ptr(enc), ptr(flat), 0, ptr(b["q"]), ptr(b["idx"]), ptr(b["counts"]), ptr(b["res"]), ptr(b["part"]), S, K, Bw, Le, B, st)
            call("wn_rvq_bwd_stats", ptr(enc), ptr(b["idx"]), ptr(b["res"]), ptr(b["d"]), ptr(flat), 0, 0.25, 1.0, ptr(b["d_out"]), ptr(b["grad"]),
                 ptr(b["stat"]), S, K, Bw, Le, B, st)
            b["state"].view(S, -1)[:, :K] = 1.0
            b["state"].view(S, -1)[:, K:] = flat.view(S, -1)
            b["state0"], b["flat0"] = b["state"].clone(), flat.clone()

    def one(name, S, which, fused):
        B, Bw, Le, K = shapes[name]
        b = bufs[name, S]
        n, kb = B * Bw * Le, K * Bw
        if which == "fwd" and fused:
            call("wn_rvq_fwd", ptr(b["enc"]), ptr(b["flat"]), 0, ptr(b["q"]), ptr(b["idx"]), ptr(b["counts"]), ptr(b["res"]), ptr(b["part"]), S, K,
                 Bw, Le, B, st)
        elif which == "fwd":                                                # S launches; r -= q_s and q += q_s in torch between them
            r, q = b["enc"], None
            for s in range(S):
                call("wn_vq_fwd", ptr(r), ptr(b["flat"]), s * kb, ptr(b["d_out"]), ptr(b["idx"], s * B * Le), ptr(b["counts"], s * K),
                     ptr(b["part"], s * _lib.VQ_NUM_PARTIALS), K, Bw, Le, B, st)
                r = torch.sub(r, b["d_out"], out=b["res"][s])
                q = b["q"].copy_(b["d_out"]) if q is None else q.add_(b["d_out"])
        elif which == "bwd" and fused:
            call("wn_rvq_bwd", ptr(b["enc"]), ptr(b["idx"]), ptr(b["res"]), ptr(b["d"]), ptr(b["flat"]), 0, 0.25, 1.0, ptr(b["d_out"]),
                 ptr(b["grad"]), S, K, Bw, Le, B, st)
        elif which == "bwd":                                                # S launches, each stage on its own input, d_enc handed on
            for s in range(S):
                call("wn_vq_bwd", ptr(b["enc"]) if s == 0 else ptr(b["res"], (s - 1) * n), ptr(b["idx"], s * B * Le),
                     ptr(b["d"]) if s == 0 else ptr(b["d_out"]), ptr(b["flat"]), s * kb, 0.25, 1.0, ptr(b["d_out"]), ptr(b["grad"]), K, Bw, Le, B, st)
        elif fused:
            call("wn_rvq_ema_update", ptr(b["flat"]), 0, ptr(b["stat"]), ptr(b["state"]), ptr(b["work"]), ptr(b["info"]), S, K, Bw, 0.99, 1e-5,
                 0.5, None, st)
        else:
            w = _lib.VQ_EMA_WORK_BYTES // 4
            for s in range(S):
                call("wn_vq_ema_update", ptr(b["flat"]), s * kb, ptr(b["stat"], s * K * (Bw + 1)), ptr(b["state"], s * K * (Bw + 1)),
                     ptr(b["work"], s * w), ptr(b["info"], 2 * s), K, Bw, 0.99, 1e-5, 0.5, None, st)

    def rounds(key, n):
        name, S, which, fused = key
        b = bufs[name, S]
        b["state"].copy_(b["state0"])
        b["flat"].copy_(b["flat0"])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(n):
            one(*key)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n * 1e3
    times = {(n, S, w, f): [] for n in shapes for S in stages for w in ("fwd", "bwd", "ema") for f in (True, False)}
    for key in times:
        rounds(key, 10)                                                       # warm
    for _ in range(alternations):
        for key in times:
            times[key].append(rounds(key, max(reps, 50)))
    for (n, S, w, f), v in times.items():
        label = "%s_%s_s%d_%s_us" % ("wn_rvq" if f else "composed", w, S, n)
        res[label], res[label + "_spread"] = _median_spread(v)
    # ---- the fused config-4 step, S = 4 against S = 1
    cfg = dict(filter_width=2, quantization_channel=256, dilations=CFG["dilations"], en_residual_channel=64, en_dilation_channel=64,
               en_bottleneck_width=64, en_pool_kernel_size=512, de_residual_channel=64, de_dilation_channel=64, de_skip_channel=256,
               use_bias=False, conditioning="learned", bottleneck="vq", vq_codes=512)
    from music_amd.faster_audio_data import onehot_device
    x = onehot_device(torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL, T)).astype(np.int32)).cuda(), 256, True)
    engs = {}
    for S in (1, 4):
        torch.manual_seed(0)
        net = wavenet_autoencoder(vq_stages=S, **cfg).cuda()
        eng = net._engine_for(torch.device("cuda", 0))
        eng.adam_init(lr=1e-4)
        with torch.no_grad():
            _, _, ws0 = eng.forward(x, None, want_probs=False, encode_only=True)
        net.init_codebook(ws0["enc_pre"], seed=0)                             # (codes in use, as in a trained model)
        engs[S] = (net, eng)
    W = T - engs[1][0].receptive_field + 1
    target = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL * W,)).astype(np.int64)).cuda()

    def steps(S, n):
        eng = engs[S][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = eng.loss_and_grad(x, target, None)
            eng.adam_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(loss)
    for S in engs:
        steps(S, 5)
    step_ms = {S: [] for S in engs}
    for _ in range(alternations):
        for S in engs:
            ms, loss = steps(S, max(reps, 20))
            step_ms[S].append(ms)
            res["fused_step_loss_s%d" % S] = round(loss, 5)
    for S, v in step_ms.items():
        res["fused_step_ms_s%d" % S], res["fused_step_ms_s%d_spread" % S] = _median_spread(v)
    res["fused_step_ms_s4_minus_s1"] = round(res["fused_step_ms_s4"] - res["fused_step_ms_s1"], 3)
    res["fused_step_ms_by_alternation"] = {"s%d" % S: [round(t, 3) for t in v] for S, v in step_ms.items()}
    stats = engs[4][1].last_vq
    res["stage_mse_s4"] = [round(float(v), 6) for v in stats.stage_mse.tolist()]
    res["stage_codes_used_s4"] = [int(v) for v in stats.stage_codes_used.tolist()]
    _write_profile("rvq_kbench.json", res)
    print(json.dumps(res))


def rvq_drop_bench(reps, alternations=6):
    """`rvq_drop`: quantiser dropout.  (a) wn_rvq_fwd_n / wn_rvq_bwd_n with every clip on all S stages against wn_rvq_fwd / wn_rvq_bwd, and
    with the stage counts of a p = 1 draw (uniform over 1 .. S), at config 4's shape (B 8, Bw 64, Le 25, K 512) and the shipped
    autoencoder's (B 4, Bw 512, Le 32, K 512), S = 4 and 8, HIP events around `reps` rounds; (b) the fused config-4 step at S = 4 with
    vq_stage_dropout = 0.5 (fresh draws every step, as ae_train makes them) against 0.  Everything alternated `alternations` times on
    one device: medians and spreads.  Written to profiles/rvq_drop_kbench.json."""
    import time
    from music_amd import _lib, vq_dropout
    from music_amd._lib import call, ptr
    from music_amd.model1 import wavenet_autoencoder
    st = _lib.stream()
    res = {"alternations": alternations}
    rng = np.random.default_rng(0)
    shapes = {"config4": (8, 64, 25, 512), "shipped": (4, 512, 32, 512)}
    stages = (4, 8)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device="cuda")
    bufs = {}
    for name, (B, Bw, Le, K) in shapes.items():
        for S in stages:
            enc = torch.from_numpy(rng.standard_normal((B, Bw, Le)).astype(np.float32)).cuda()
            flat = torch.from_numpy(np.concatenate([rng.standard_normal(K * Bw) * 0.8 ** s for s in range(S)]).astype(np.float32)).cuda()
            drawn = vq_dropout.draw_stages(0, 0, 0, B, S, 1.0)
            bufs[name, S] = dict(enc=enc, flat=flat, q=f32(B, Bw, Le), idx=i32(S, B, Le), counts=i32(S, K), res=f32(S, B, Bw, Le),
                                 part=f32(S, _lib.VQ_NUM_PARTIALS), d=torch.randn_like(enc), d_out=f32(B, Bw, Le), grad=torch.empty_like(flat),
                                 n_all=torch.full((B,), S, dtype=torch.int32, device="cuda"), n_drawn=torch.from_numpy(drawn).cuda())
            res["drawn_counts_%s_s%d" % (name, S)] = drawn.tolist()

    def one(name, S, which, form):
        B, Bw, Le, K = shapes[name]
        b = bufs[name, S]
        n = None if form == "plain" else b["n_all" if form == "all" else "n_drawn"]
        if which == "fwd" and n is None:
            call("wn_rvq_fwd", ptr(b["enc"]), ptr(b["flat"]), 0, ptr(b["q"]), ptr(b["idx"]), ptr(b["counts"]), ptr(b["res"]), ptr(b["part"]), S, K,
                 Bw, Le, B, st)
        elif which == "fwd":
            call("wn_rvq_fwd_n", ptr(b["enc"]), ptr(b["flat"]), 0, ptr(n), ptr(b["q"]), ptr(b["idx"]), ptr(b["counts"]), ptr(b["res"]),
                 ptr(b["part"]), S, K, Bw, Le, B, st)
        elif n is None:
            call("wn_rvq_bwd", ptr(b["enc"]), ptr(b["idx"]), ptr(b["res"]), ptr(b["d"]), ptr(b["flat"]), 0, 0.25, 1.0, ptr(b["d_out"]),
                 ptr(b["grad"]), S, K, Bw, Le, B, st)
        else:
            call("wn_rvq_bwd_n", ptr(b["enc"]), ptr(b["idx"]), ptr(b["res"]), ptr(n), ptr(b["d"]), ptr(b["flat"]), 0, 0.25, 1.0, ptr(b["d_out"]),
                 ptr(b["grad"]), S, K, Bw, Le, B, st)

    def rounds(key, n):
        name, S, which, form = key
        if which == "bwd":                                                    # the backward reads the idx and res of ITS forward
            one(name, S, "fwd", form)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(n):
            one(*key)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n * 1e3
    times = {(n, S, w, f): [] for n in shapes for S in stages for w in ("fwd", "bwd") for f in ("plain", "all", "drawn")}
    for key in times:
        rounds(key, 10)                                                       # warm
    for _ in range(alternations):
        for key in times:
            times[key].append(rounds(key, max(reps, 50)))
    for (n, S, w, f), v in times.items():
        label = "%s_%s_s%d_%s_us" % ({"plain": "wn_rvq", "all": "wn_rvq_n_all", "drawn": "wn_rvq_n_drawn"}[f], w, S, n)
        res[label], res[label + "_spread"] = _median_spread(v)
    for n in shapes:
        for S in stages:
            for w in ("fwd", "bwd"):
                plain = res["wn_rvq_%s_s%d_%s_us" % (w, S, n)]
                for f in ("all", "drawn"):
                    res["ratio_n_%s_over_plain_%s_s%d_%s" % (f, w, S, n)] = round(res["wn_rvq_n_%s_%s_s%d_%s_us" % (f, w, S, n)] / plain, 4)
    # ---- the fused config-4 step at S = 4, p = 0.5 against p = 0
    cfg = dict(filter_width=2, quantization_channel=256, dilations=CFG["dilations"], en_residual_channel=64, en_dilation_channel=64,
               en_bottleneck_width=64, en_pool_kernel_size=512, de_residual_channel=64, de_dilation_channel=64, de_skip_channel=256,
               use_bias=False, conditioning="learned", bottleneck="vq", vq_codes=512, vq_stages=4)
    from music_amd.faster_audio_data import onehot_device
    x = onehot_device(torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL, T)).astype(np.int32)).cuda(), 256, True)
    engs = {}
    for p in (0.0, 0.5):
        torch.manual_seed(0)
        net = wavenet_autoencoder(vq_stage_dropout=p, **cfg).cuda()
        eng = net._engine_for(torch.device("cuda", 0))
        eng.adam_init(lr=1e-4)
        with torch.no_grad():
            _, _, ws0 = eng.forward(x, None, want_probs=False, encode_only=True)
        net.init_codebook(ws0["enc_pre"], seed=0)                             # (codes in use, as in a trained model)
        engs[p] = (net, eng)
    W = T - engs[0.0][0].receptive_field + 1
    target = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL * W,)).astype(np.int64)).cuda()
    step_no = {p: 0 for p in engs}

    def steps(p, n):
        net, eng = engs[p]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            drawn = net.draw_stages(B_LOCAL, step=step_no[p])                 # None at p = 0: the launches without dropout
            step_no[p] += 1
            loss = eng.loss_and_grad(x, target, None, stages=drawn)
            eng.adam_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(loss)
    for p in engs:
        steps(p, 5)
    step_ms = {p: [] for p in engs}
    for _ in range(alternations):
        for p in engs:
            ms, loss = steps(p, max(reps, 20))
            step_ms[p].append(ms)
            res["fused_step_loss_p%g" % p] = round(loss, 5)
    for p, v in step_ms.items():
        res["fused_step_ms_p%g" % p], res["fused_step_ms_p%g_spread" % p] = _median_spread(v)
    res["fused_step_ms_p0.5_minus_p0"] = round(res["fused_step_ms_p0.5"] - res["fused_step_ms_p0"], 3)
    res["fused_step_ms_by_alternation"] = {"p%g" % p: [round(t, 3) for t in v] for p, v in step_ms.items()}
    stats = engs[0.5][1].last_vq
    res["stage_frames_last_step_p0.5"] = [int(v) for v in stats.stage_frames.tolist()]
    _write_profile("rvq_drop_kbench.json", res)
    print(json.dumps(res))


def gcond_bench(reps, alternations=6, E=64, n_cls=8):
    """`gcond`: global class conditioning.  (a) wn_gcond_proj_fwd / _bwd beside wn_cond_proj_fwd / _bwd, whose place they take, alone
    at config 4's shape and at the shipped autoencoder's with E = 64 channels, HIP events around `reps` calls; (b) the fused config-4
    step of a global model against the learned model; everything alternated `alternations` times on one device, medians and spreads
    (largest - smallest).  Written to profiles/gcond_kbench.json."""
    import time
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.model1 import wavenet_autoencoder
    st = _lib.stream()
    res = {"alternations": alternations, "E": E, "n_cls": n_cls}
    rng = np.random.default_rng(0)
    shapes = {"config4": dict(N=30, Dd=64, CH=64, Sd=256, Bw=64, Le=25, B=8, pair=False),
              "shipped": dict(N=40, Dd=32, CH=32, Sd=512, Bw=512, Le=32, B=4, pair=True)}
    legs = {}
    for tag, g in shapes.items():
        N, Dd, CH, Sd, Bw, Le, B, pair = (g[k] for k in ("N", "Dd", "CH", "Sd", "Bw", "Le", "B", "pair"))
        rnd = lambda *shape: torch.randn(*shape, device="cuda")
        stride = 2 * Dd * Bw + 2 * Dd
        n_l = N * stride + Sd * Bw + Sd
        n = n_l + N * 2 * Dd * E + Sd * E + n_cls * E
        flat, grad, enc = rnd(n) * 0.1, torch.empty(n, device="cuda"), rnd(B, Bw, Le)
        offs = (0, 2 * Dd * Bw, stride, N * stride, N * stride + Sd * Bw)
        goffs = (n_l, 2 * Dd * E, n_l + N * 2 * Dd * E, n_l + N * 2 * Dd * E + Sd * E, E, n_cls)
        dims = (N, Dd, CH, Sd, Bw, Le, B)
        tab, tabp, enf = rnd(N, B, 2 * CH, Le), (rnd(N, B // 2, 4 * CH, Le) if pair else None), rnd(B, Sd, Le)
        d_enc = torch.empty(B, Bw, Le, device="cuda")
        cls = torch.from_numpy((np.arange(B) % n_cls).astype(np.int32)).cuda()
        fwd = (ptr(enc), ptr(flat)) + offs + (ptr(tab), ptr(tabp), ptr(enf)) + dims
        bwd = (ptr(tabp if pair else tab), 1 if pair else 0, ptr(enf), ptr(enc), ptr(flat)) + offs + (ptr(d_enc), ptr(grad)) + dims
        keep = (flat, grad, enc, tab, tabp, enf, d_enc, cls)
        legs[(tag, "cond_fwd")] = (lambda a=fwd, k=keep: call("wn_cond_proj_fwd", *a, st))
        legs[(tag, "cond_bwd")] = (lambda a=bwd, k=keep: call("wn_cond_proj_bwd", *a, st))
        legs[(tag, "gcond_fwd")] = (lambda a=fwd + (ptr(cls),) + goffs, k=keep: call("wn_gcond_proj_fwd", *a, st))
        legs[(tag, "gcond_bwd")] = (lambda a=bwd + (ptr(cls),) + goffs, k=keep: call("wn_gcond_proj_bwd", *a, st))
        res["shape_" + tag] = g

    def launches(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n * 1e3
    times = {key: [] for key in legs}
    for key, fn in legs.items():
        launches(fn, 20)                                                      # warm
    for _ in range(alternations):
        for key, fn in legs.items():
            times[key].append(launches(fn, max(reps, 100)))
    for (tag, leg), v in times.items():
        res["wn_%s_%s_us" % (leg.replace("_", "_proj_"), tag)], res["wn_%s_%s_us_spread" % (leg.replace("_", "_proj_"), tag)] = _median_spread(v)
    # ---- the fused config-4 step
    cfg = dict(filter_width=2, quantization_channel=256, dilations=CFG["dilations"], en_residual_channel=64, en_dilation_channel=64,
               en_bottleneck_width=64, en_pool_kernel_size=512, de_residual_channel=64, de_dilation_channel=64, de_skip_channel=256,
               use_bias=False, conditioning="learned")
    codes = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL, T)).astype(np.int32)).cuda()
    from music_amd.faster_audio_data import onehot_device
    x = onehot_device(codes, 256, True)
    engs = {}
    for mode, kw in (("learned", {}), ("global", dict(global_classes=n_cls, global_channels=E))):
        torch.manual_seed(0)
        net = wavenet_autoencoder(**dict(cfg, **kw)).cuda()
        eng = net._engine_for(torch.device("cuda", 0))
        eng.adam_init(lr=1e-4)
        engs[mode] = eng
    W = T - engs["global"].rf + 1
    target = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL * W,)).astype(np.int64)).cuda()
    classes = torch.arange(B_LOCAL, dtype=torch.int64) % n_cls               # on the host, as the loader hands them on

    def steps(mode, n):
        eng = engs[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = eng.loss_and_grad(x, target, None, classes=classes if mode == "global" else None)
            eng.adam_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(loss)
    for mode in engs:
        steps(mode, 5)
    step_ms = {m: [] for m in engs}
    for _ in range(alternations):
        for mode in engs:
            ms, loss = steps(mode, max(reps, 20))
            step_ms[mode].append(ms)
            res["fused_step_loss_" + mode] = round(loss, 5)
    for mode, v in step_ms.items():
        res["fused_step_ms_" + mode], res["fused_step_ms_%s_spread" % mode] = _median_spread(v)
    res["fused_step_ms_global_minus_learned"] = round(res["fused_step_ms_global"] - res["fused_step_ms_learned"], 3)
    res["fused_step_ms_by_alternation"] = {m: [round(t, 3) for t in v] for m, v in step_ms.items()}
    res["shape_config4_step"] = dict(B=B_LOCAL, T=T, Le=W // 512, Bw=64, E=E, n_cls=n_cls)
    _write_profile("gcond_kbench.json", res)
    print(json.dumps(res))


def gclass_bench(reps, alternations=6, E=64, n_cls=8):
    """`gclass`: the class-conditional WaveNet.  (a) wn_gclass_fwd / wn_gclass_bwd alone at config 2's shape (30 blocks, 64 / 256
    channels, 8 clips) with E = 64 channels, HIP events around max(reps, 100) calls; (b) the fused step (forward, loss, backward, flat
    Adam) conditioned against unconditioned at config 2's shape (the fast engine: the conditioned one runs the three-launch forward
    epilogue) and at a prior's (8 x 1024 x 4096, the general plan); everything alternated `alternations` times on one device, medians
    and spreads (largest - smallest).  Written to profiles/gclass_kbench.json."""
    import time
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.faster_audio_data import onehot_device
    from music_amd.model import wavenet
    st = _lib.stream()
    res = {"alternations": alternations, "E": E, "n_cls": n_cls}
    rng = np.random.default_rng(0)
    N, D, CH, S, B = len(CFG["dilations"]), 64, 64, 256, B_LOCAL
    n = N * 2 * D * E + S * E + n_cls * E
    flat, grad = torch.randn(n, device="cuda") * 0.1, torch.empty(n, device="cuda")
    goffs = (0, 2 * D * E, N * 2 * D * E, N * 2 * D * E + S * E, E, n_cls)
    tab, tabp, enf = torch.randn(N, B, 2 * CH, device="cuda"), torch.randn(N, B // 2, 4 * CH, device="cuda"), torch.randn(B, S, device="cuda")
    cls = torch.from_numpy((np.arange(B) % n_cls).astype(np.int32)).cuda()
    legs = {"gclass_fwd": lambda: call("wn_gclass_fwd", ptr(flat), ptr(tab), None, ptr(enf), N, D, CH, S, B, ptr(cls), *goffs, st),
            "gclass_fwd_both_tables": lambda: call("wn_gclass_fwd", ptr(flat), ptr(tab), ptr(tabp), ptr(enf), N, D, CH, S, B, ptr(cls), *goffs, st),
            "gclass_bwd": lambda: call("wn_gclass_bwd", ptr(tab), 0, ptr(enf), ptr(flat), ptr(grad), N, D, CH, S, B, ptr(cls), *goffs, st)}
    res["shape_kernels"] = dict(N=N, D=D, CH=CH, S=S, B=B)

    def launches(fn, k):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(k):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / k * 1e3
    times = {key: [] for key in legs}
    for fn in legs.values():
        launches(fn, 20)                                                      # warm
    for _ in range(alternations):
        for key, fn in legs.items():
            times[key].append(launches(fn, max(reps, 100)))
    for leg, v in times.items():
        res["wn_%s_us" % leg], res["wn_%s_us_spread" % leg] = _median_spread(v)
    # ---- the fused step, conditioned against unconditioned
    shapes = {"config2": (dict(CFG), B_LOCAL, T), "prior_8x1024x4096": (dict(CFG, quantization_channels=1024), 8, 4096)}
    for tag, (cfg, Bs, Ts) in shapes.items():
        Q = cfg["quantization_channels"]
        codes = torch.from_numpy(rng.integers(0, Q, size=(Bs, Ts)).astype(np.int32)).cuda()
        x = onehot_device(codes, Q, True)
        engs = {}
        for mode, kw in (("plain", {}), ("classes", dict(global_classes=n_cls, global_channels=E))):
            torch.manual_seed(0)
            net = wavenet(**dict(cfg, **kw)).cuda()
            eng = net._engine_for(torch.device("cuda", 0))
            eng.adam_init(lr=1e-4)
            engs[mode] = eng
        W = Ts - engs["plain"].rf + 1
        target = torch.from_numpy(rng.integers(0, Q, size=(Bs * W,)).astype(np.int64)).cuda()
        classes = torch.arange(Bs, dtype=torch.int64) % n_cls                 # on the host, as the loader hands them on

        def steps(mode, k):
            eng = engs[mode]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                loss = eng.loss_and_grad(x, target, **({"classes": classes} if mode == "classes" else {}))
                eng.adam_step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / k * 1e3, float(loss)
        for mode in engs:
            steps(mode, 5)
        step_ms = {m: [] for m in engs}
        for _ in range(alternations):
            for mode in engs:
                ms, loss = steps(mode, max(reps, 20))
                step_ms[mode].append(ms)
                res["%s_fused_step_loss_%s" % (tag, mode)] = round(loss, 5)
        for mode, v in step_ms.items():
            res["%s_fused_step_ms_%s" % (tag, mode)], res["%s_fused_step_ms_%s_spread" % (tag, mode)] = _median_spread(v)
        res["%s_fused_step_ms_classes_minus_plain" % tag] = round(res["%s_fused_step_ms_classes" % tag] - res["%s_fused_step_ms_plain" % tag], 3)
        res["%s_fused_step_ms_by_alternation" % tag] = {m: [round(t, 3) for t in v] for m, v in step_ms.items()}
        res["shape_" + tag] = dict(B=Bs, T=Ts, Q=Q, engine=type(engs["classes"]).__name__, E=E, n_cls=n_cls)
        del engs, x, target
        torch.cuda.empty_cache()
    _write_profile("gclass_kbench.json", res)
    print(json.dumps(res))


def phase_bench(reps, alternations=6, P=4):
    """`phase`: the phase-conditioned WaveNet.  (a) wn_phase_tab_fwd / wn_phase_tab_bwd alone at a prior's shape (8 clips, 30 blocks,
    64 / 256 channels, P = 4; the forward with one and with both table layouts, the backward without and with the frame sums), HIP
    events around max(reps, 100) calls; (b) the fused step (forward, loss, backward, flat Adam) with phase_period = 4 against the plain
    model at a prior's 8 x 512 x 4096 (the general plan) and at config 2's shape (the fast plan: the conditioned one runs the
    three-launch forward epilogue); everything alternated `alternations` times on one device, medians and spreads (largest -
    smallest).  Written to profiles/phase_kbench.json."""
    import time
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.faster_audio_data import onehot_device
    from music_amd.model import wavenet
    st = _lib.stream()
    res = {"alternations": alternations, "P": P}
    rng = np.random.default_rng(0)
    N, D, CH, S, B = len(CFG["dilations"]), 64, 64, 256, 8
    n = (N * 2 * D + S) * P
    flat, grad = torch.randn(n, device="cuda") * 0.1, torch.empty(n, device="cuda")
    offs = (0, 2 * D * P, N * 2 * D * P)
    tab, tabp, enf = torch.randn(N, B, 2 * CH, P, device="cuda"), torch.randn(N, B // 2, 4 * CH, P, device="cuda"), torch.randn(B, S, P, device="cuda")
    s_tab, s_enf = torch.empty(N, B, 2 * CH, device="cuda"), torch.empty(B, S, device="cuda")
    pos = torch.from_numpy(rng.integers(0, 1 << 40, size=B).astype(np.int64)).cuda()
    rot = torch.from_numpy(rng.integers(0, P, size=N + 1).astype(np.int32)).cuda()
    dims = (N, D, CH, S, P, B)
    head = (ptr(flat),) + offs + (ptr(pos), ptr(rot))
    legs = {"phase_tab_fwd": lambda: call("wn_phase_tab_fwd", *head, None, None, None, ptr(tab), None, ptr(enf), *dims, st),
            "phase_tab_fwd_both_tables": lambda: call("wn_phase_tab_fwd", *head, None, None, None, ptr(tab), ptr(tabp), ptr(enf), *dims, st),
            "phase_tab_fwd_class_addends": lambda: call("wn_phase_tab_fwd", *head, ptr(s_tab), None, ptr(s_enf), ptr(tab), None, ptr(enf), *dims, st),
            "phase_tab_bwd": lambda: call("wn_phase_tab_bwd", ptr(tab), 0, ptr(enf), ptr(grad), *offs, ptr(pos), ptr(rot), None, None, *dims, st),
            "phase_tab_bwd_frame_sums": lambda: call("wn_phase_tab_bwd", ptr(tab), 0, ptr(enf), ptr(grad), *offs, ptr(pos), ptr(rot), ptr(s_tab),
                                                     ptr(s_enf), *dims, st)}
    s_tab.normal_()
    s_enf.normal_()
    res["shape_kernels"] = dict(N=N, D=D, CH=CH, S=S, B=B, P=P)

    def launches(fn, k):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(k):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / k * 1e3
    times = {key: [] for key in legs}
    for fn in legs.values():
        launches(fn, 20)                                                      # warm
    for _ in range(alternations):
        for key, fn in legs.items():
            times[key].append(launches(fn, max(reps, 100)))
    for leg, v in times.items():
        res["wn_%s_us" % leg], res["wn_%s_us_spread" % leg] = _median_spread(v)
    # ---- the fused step, phase-conditioned against plain
    shapes = {"prior_8x512x4096": (dict(CFG, quantization_channels=512), 8, 4096), "config2": (dict(CFG), B_LOCAL, T)}
    for tag, (cfg, Bs, Ts) in shapes.items():
        Q = cfg["quantization_channels"]
        codes = torch.from_numpy(rng.integers(0, Q, size=(Bs, Ts)).astype(np.int32)).cuda()
        x = onehot_device(codes, Q, True)
        engs = {}
        for mode, kw in (("plain", {}), ("phase", dict(phase_period=P))):
            torch.manual_seed(0)
            net = wavenet(**dict(cfg, **kw)).cuda()
            eng = net._engine_for(torch.device("cuda", 0))
            eng.adam_init(lr=1e-4)
            engs[mode] = eng
        W = Ts - engs["plain"].rf + 1
        target = torch.from_numpy(rng.integers(0, Q, size=(Bs * W,)).astype(np.int64)).cuda()
        ppos = torch.from_numpy(rng.integers(0, 1 << 20, size=Bs).astype(np.int64)).cuda()       # on the device, as the loader hands them on

        def steps(mode, k):
            eng = engs[mode]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                loss = eng.loss_and_grad(x, target, **({"phase_pos": ppos} if mode == "phase" else {}))
                eng.adam_step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / k * 1e3, float(loss)
        for mode in engs:
            steps(mode, 5)
        step_ms = {m: [] for m in engs}
        for _ in range(alternations):
            for mode in engs:
                ms, loss = steps(mode, max(reps, 20))
                step_ms[mode].append(ms)
                res["%s_fused_step_loss_%s" % (tag, mode)] = round(loss, 5)
        for mode, v in step_ms.items():
            res["%s_fused_step_ms_%s" % (tag, mode)], res["%s_fused_step_ms_%s_spread" % (tag, mode)] = _median_spread(v)
        res["%s_fused_step_ms_phase_minus_plain" % tag] = round(res["%s_fused_step_ms_phase" % tag] - res["%s_fused_step_ms_plain" % tag], 3)
        res["%s_fused_step_ms_by_alternation" % tag] = {m: [round(t, 3) for t in v] for m, v in step_ms.items()}
        res["shape_" + tag] = dict(B=Bs, T=Ts, Q=Q, engine=type(engs["phase"]).__name__, P=P)
        del engs, x, target
        torch.cuda.empty_cache()
    _write_profile("phase_kbench.json", res)
    print(json.dumps(res))


def win_nll_bench(reps, alternations=6):
    """`win_nll`: the windowed objective's launch (wn_win_step_nll) against the plain one (wn_step_nll, the yardstick: the kernel from
    before the windows, measured in the same run) on random logits, with dx and forward-only (row_nll + row_hit), at config 2's shape
    (8 x 256 x 12930, windows 4 x 64: the q = 256 instantiation) and at a prior's (8 x 1024 x 4096, windows 4 x 256: the q > 512 one).
    HIP events around `reps * 20` back-to-back launches, the legs alternated `alternations` times on one device: medians and spreads
    (largest - smallest).  Written to profiles/win_nll_kbench.json."""
    import ctypes
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.fast_generate import stage_windows
    st = _lib.stream()
    res = {"what": "wn_win_step_nll against wn_step_nll in one run, %d launches per timing, %d alternations; us" % (reps * 20, alternations)}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, (B, Q, W, stages) in (("config2_8x256x12930_4x64", (B_LOCAL, 256, T - 3070, 4)), ("prior_8x1024x4096_4x256", (8, 1024, 4096, 4))):
        K = Q // stages
        n = B * W
        x = torch.randn(B * Q * W, device="cuda", generator=g)
        pos = torch.randint(0, 1 << 20, (B,), device="cuda", generator=g)
        col = pos.view(B, 1) + torch.arange(W, device="cuda").view(1, W)
        target = ((col % stages) * K + torch.randint(0, K, (B, W), device="cuda", generator=g)).reshape(-1).contiguous()
        dx = torch.empty_like(x)
        part = torch.zeros(_lib.CE_NUM_PARTIALS, device="cuda")
        row_nll = torch.empty(n, dtype=torch.float32, device="cuda")
        row_hit = torch.empty(n, dtype=torch.int32, device="cuda")
        host = (ctypes.c_int32 * (2 * stages))(*[v for pr in stage_windows(stages, K) for v in pr])
        tail = (ctypes.cast(host, ctypes.c_void_p), stages, ptr(pos), 0)
        head_dx = (ptr(x), Q * W, W, ptr(target), ptr(dx), Q * W, W, None, None, None, ptr(part), W, Q, B, 1.0 / n)
        head_sc = (ptr(x), Q * W, W, ptr(target), None, 0, 0, None, ptr(row_nll), ptr(row_hit), ptr(part), W, Q, B, 1.0 / n)
        legs = {
            "step_nll": lambda: call("wn_step_nll", *head_dx, st),
            "win_step_nll": lambda: call("wn_win_step_nll", *head_dx, *tail, st),
            "step_nll_score": lambda: call("wn_step_nll", *head_sc, st),
            "win_step_nll_score": lambda: call("wn_win_step_nll", *head_sc, *tail, st),
        }

        def timed(fn):
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps * 20):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / (reps * 20) * 1e3
        us = {k: [] for k in legs}
        for _ in range(alternations):
            for k, fn in legs.items():
                us[k].append(timed(fn))
        assert not bool(torch.isnan(part.sum()))                     # (the targets respect the windows: a poisoned run measures nothing)
        r = {"shape": [B, Q, W], "windows": [stages, K], "algorithmic_bytes_with_dx": 2 * B * Q * W * 4}
        for k, vals in us.items():
            r[k + "_us"], r[k + "_us_spread"] = _median_spread(vals)
            r[k + "_us_all"] = [round(v, 2) for v in vals]
        r["win_over_plain"] = round(r["win_step_nll_us"] / r["step_nll_us"], 3)
        r["win_over_plain_score"] = round(r["win_step_nll_score_us"] / r["step_nll_score_us"], 3)
        res[label] = r
    _write_profile("win_nll_kbench.json", res)
    print(json.dumps(res))


def wnll_bench(reps, alternations=6):
    """`wnll`: the masked / weighted / smoothed objective's entry (wn_wstep_nll: the denominator's launch and the main kernel, both
    inside the timing) against wn_win_step_nll, the entry from before, on identical logits with dx, at a prior's shape (8 x 512 x 4096,
    windows 4 x 128: the q <= 512 instantiation) and at config 2's (8 x 256 x 12930, windows 4 x 64: the q = 256 one).  Variants:
    unmasked (the degenerate call: the same arithmetic as the old entry), half the columns ignored, smoothing 0.1.  HIP events around
    `reps * 20` back-to-back calls, the legs alternated `alternations` times on one device: medians and spreads (largest - smallest).
    Written to profiles/wnll_kbench.json."""
    import ctypes
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.fast_generate import stage_windows
    st = _lib.stream()
    calls = reps * 20
    res = {"what": "wn_wstep_nll (nll_den_k + step_nll_k) against wn_win_step_nll in one run, %d back-to-back calls per timing, "
                   "%d alternations; us per call" % (calls, alternations)}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, (B, Q, W, stages) in (("prior_8x512x4096_4x128", (8, 512, 4096, 4)), ("config2_8x256x12930_4x64", (B_LOCAL, 256, T - 3070, 4))):
        K = Q // stages
        n = B * W
        x = torch.randn(B * Q * W, device="cuda", generator=g)
        pos = torch.randint(0, 1 << 20, (B,), device="cuda", generator=g)
        col = pos.view(B, 1) + torch.arange(W, device="cuda").view(1, W)
        target = ((col % stages) * K + torch.randint(0, K, (B, W), device="cuda", generator=g)).reshape(-1).contiguous()
        half = torch.where(torch.rand(n, device="cuda", generator=g) < 0.5, target, torch.full_like(target, -1))
        dx = torch.empty_like(x)
        part = torch.zeros(_lib.CE_NUM_PARTIALS, device="cuda")
        den = torch.zeros(2, device="cuda")
        host = (ctypes.c_int32 * (2 * stages))(*[v for pr in stage_windows(stages, K) for v in pr])
        tail = (ctypes.cast(host, ctypes.c_void_p), stages, ptr(pos), 0)
        head = lambda t: (ptr(x), Q * W, W, ptr(t), ptr(dx), Q * W, W, None, None, None, ptr(part), W, Q, B)
        legs = {
            "win_step_nll": lambda: call("wn_win_step_nll", *head(target), 1.0 / n, *tail, st),
            "wstep_nll_unmasked": lambda: call("wn_wstep_nll", *head(target), *tail, None, -1, 0.0, ptr(den), st),
            "wstep_nll_half_masked": lambda: call("wn_wstep_nll", *head(half), *tail, None, -1, 0.0, ptr(den), st),
            "wstep_nll_smoothing": lambda: call("wn_wstep_nll", *head(target), *tail, None, -1, 0.1, ptr(den), st),
        }

        def timed(fn):
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(calls):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / calls * 1e3
        us = {k: [] for k in legs}
        for _ in range(alternations):
            for k, fn in legs.items():
                us[k].append(timed(fn))
        assert not bool(torch.isnan(part.sum()))                     # (the targets respect the windows: a poisoned run measures nothing)
        r = {"shape": [B, Q, W], "windows": [stages, K], "algorithmic_bytes": 2 * B * Q * W * 4, "extra_bytes_per_column": 4}
        for k, vals in us.items():
            r[k + "_us"], r[k + "_us_spread"] = _median_spread(vals)
            r[k + "_us_all"] = [round(v, 2) for v in vals]
        for k in list(legs)[1:]:
            r[k + "_over_old"] = round(r[k + "_us"] / r["win_step_nll_us"], 3)
        res[label] = r
    _write_profile("wnll_kbench.json", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="f16x3,bf16x3")
    ap.add_argument("--overlap", type=int, default=1)
    ap.add_argument("--parent", default=None, help="gcond / gclass / phase / rvq / rvq_drop / win_nll / wnll: a built checkout of the parent commit, for profiles/<what>_bench_unset.json")
    args = ap.parse_args()
    if args.what == "gcond":
        if args.parent:
            bench_unset(os.path.abspath(args.parent))
        return gcond_bench(args.reps)
    if args.what == "gclass":
        if args.parent:
            bench_unset(os.path.abspath(args.parent), profile="gclass_bench_unset.json", keys="global_classes / global_channels of wavenet")
        return gclass_bench(args.reps)
    if args.what == "phase":
        if args.parent:
            bench_unset(os.path.abspath(args.parent), profile="phase_bench_unset.json", keys="phase_period of wavenet")
        return phase_bench(args.reps)
    if args.what == "rvq":
        if args.parent:
            bench_unset(os.path.abspath(args.parent), profile="rvq_bench_unset.json", keys="vq_stages")
        return rvq_bench(args.reps)
    if args.what == "rvq_drop":
        if args.parent:
            bench_unset(os.path.abspath(args.parent), profile="rvq_drop_bench_unset.json", keys="vq_stage_dropout")
        return rvq_drop_bench(args.reps)
    if args.what == "win_nll":
        if args.parent:
            bench_unset(os.path.abspath(args.parent), profile="win_nll_bench_unset.json", keys="nll_windows / token_positions")
        return win_nll_bench(args.reps)
    if args.what == "wnll":
        if args.parent:
            bench_unset(os.path.abspath(args.parent), profile="wnll_bench_unset.json", keys="ignore_token / label_smoothing / nll_stage_weights")
        return wnll_bench(args.reps)
    if args.what == "vq":
        return vq_bench(args.reps)
    if args.what == "vq_ema":
        return vq_ema_bench(args.reps)
    from music_amd.model import wavenet
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.engine import SLACK
    torch.manual_seed(0)
    net = wavenet(**CFG)
    net.precision = tuple(args.precision.split(","))
    net = net.cuda()
    eng = net._engine_for(torch.device("cuda", 0))
    eng.overlap_wgrad = bool(args.overlap)
    rng = np.random.default_rng(0)
    codes = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL, T)).astype(np.int32)).cuda()
    target = torch.from_numpy(rng.integers(0, 256, size=(B_LOCAL * (T - 3070),)).astype(np.int64)).cuda()
    x = eng.onehot(codes)
    for _ in range(2):
        eng.loss_and_grad(x, target)
    torch.cuda.synchronize()
    ws = eng.workspace(B_LOCAL, T)
    st = _lib.stream()
    CH, N, pitch = eng.CH, eng.N, ws["pitch"]
    xb, zb = CH * pitch, N * CH * pitch
    fr = lambda name: ptr(eng.pk_f, eng.pk_f_off[name])
    res = {}
    if args.what in ("fwd", "all"):
        per_layer = []
        for i, d in enumerate(eng.dil):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.reps):
                call("wn_resblock_fwd", eng._x(ws, i), eng._x(ws, i + 1), ptr(ws["Z"], SLACK + i * CH * pitch), xb, zb, pitch,
                     fr("fg%d" % i), fr("d%d" % i), None, None, None, eng.D, eng.R, CH, d, eng.off[i + 1], T, eng.rf - 1,
                     1, None, 0, 0, 0, 0, 0, None, 0, None, 0, B_LOCAL, eng.mode_fwd, st)
            ev[1].record()
            torch.cuda.synchronize()
            per_layer.append(ev[0].elapsed_time(ev[1]) / args.reps * 1e3)
        res["resblock_fwd_us_by_layer"] = [round(v, 1) for v in per_layer]
        res["resblock_fwd_us_total"] = round(sum(per_layer), 1)
    if args.what == "dx":
        # the per-layer data-gradient product in isolation, and cut-down forms of it (timing only)
        eng.loss_and_grad(x, target)
        bw = ws["bwd"]
        i = 12
        d, t_lo = eng.dil[i], eng.off[i + 1]
        dfg = ptr(bw["dfg"][0], SLACK)
        dy = ptr(bw["dX"][1], SLACK)
        out = ptr(bw["dX"][0], SLACK)
        br = lambda name: ptr(eng.pk_b, eng.pk_b_off[name])

        def run(ks0, ks1, resid, label, shift=d, in_hi=pitch):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(args.reps):
                call("wn_chan_gemm", dfg, dfg if ks1 else None, 2 * CH * pitch, pitch, t_lo, in_hi, 0, shift, ks0, ks1, br("fgT%d" % i),
                     CH // 16, eng.R, out, xb, pitch, 0, None, dy if resid else None, xb, pitch, t_lo, None, 0, 0, eng.off[i], T, 0,
                     B_LOCAL, eng.mode_bwd, st)
            ev[1].record()
            torch.cuda.synchronize()
            res[label] = round(ev[0].elapsed_time(ev[1]) / args.reps * 1e3, 1)
        run(4, 4, True, "dx_full_us")
        run(4, 4, False, "dx_noresid_us")
        run(4, 0, True, "dx_one_tap_us")
        run(2, 0, True, "dx_half_tap_us")
        run(1, 0, False, "dx_one_kstep_noresid_us")
        run(4, 4, True, "dx_shift0_us", shift=0)
        res["layer"] = dict(i=i, d=d, t_lo=t_lo)
    if args.what == "skip":
        # the skip product (wide GEMM, K = 1920) in isolation with shortened K (timing only)
        eng.loss_and_grad(x, target)
        lo, SP = eng.rf - 1, eng.SP

        def run(ks, label):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(args.reps):
                call("wn_chan_gemm", ptr(ws["Z"], SLACK), None, zb, pitch, lo, T, 0, 0, ks, 0, fr("skip"), SP // 16, eng.S,
                     ptr(ws["U"], SLACK), SP * pitch, pitch, 0, None, None, 0, 0, 0, None, 0, 0, lo, T, 0, B_LOCAL, eng.mode_fwd, st)
            ev[1].record()
            torch.cuda.synchronize()
            res[label] = round(ev[0].elapsed_time(ev[1]) / args.reps * 1e3, 1)
        for ks in (60, 30, 15, 8, 2):
            run(ks, "skip_ks%d_us" % ks)
    if args.what in ("bwd", "all", "epi"):
        eng.fine_marks = args.what == "epi"
        eng.marks = []
        for _ in range(args.reps):
            eng.loss_and_grad(x, target)
        torch.cuda.synchronize()
        marks, eng.marks = eng.marks, None
        ph = {}
        for (n0, e0), (n1, e1) in zip(marks[:-1], marks[1:]):
            ph[n1] = ph.get(n1, 0.0) + e0.elapsed_time(e1)
        res["phase_ms"] = {k: round(v / args.reps, 3) for k, v in ph.items() if k != "begin"}
    if args.what in ("decode", "all"):
        # BASELINE config 5: 30-layer model, class-128 start piece, 1 s of 16 kHz audio, greedy
        import time
        from music_amd import fast_generate as fg
        start = torch.zeros(1, 256, net.receptive_field, device="cuda")
        start[:, 128, :] = 1.0
        fg.generate_codes(net, start, 200)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = fg.generate_codes(net, start, 16000)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res["decode_16000_samples_s"] = round(dt, 4)
        res["decode_samples_per_s"] = round(16000 / dt, 1)
        res["decode_distinct_codes"] = int(torch.unique(codes).numel())
        # batched utterances: U independent streams in one launch
        for U in (16, 64, 128, 512, 1024):
            starts = start.repeat(U, 1, 1).clone()
            for u in range(U):                      # different start classes so the streams differ
                starts[u].zero_()
                starts[u, (128 + u) % 256, :] = 1.0
            fg.generate_codes_batch(net, starts, 50)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cb = fg.generate_codes_batch(net, starts, 4000)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res["decode_batch%d_samples_per_s" % U] = round(U * 4000 / dt, 1)
        # the same model with biases (what the autoencoder's cached decoder looks like to the kernel)
        from music_amd.model import wavenet as _wn
        torch.manual_seed(1)
        netb = _wn(**dict(CFG, use_bias=True)).cuda()
        fg.generate_codes(netb, start, 200)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fg.generate_codes(netb, start, 8000)
        torch.cuda.synchronize()
        res["decode_bias_samples_per_s"] = round(8000 / (time.perf_counter() - t0), 1)
    if args.what == "guard":
        # the guarded optimizer step on config 2's flat buffers: wn_grad_guard (two launches) and the guarded Adam against the plain
        # one, by HIP events over `reps` back-to-back calls; then the whole fused step guarded / unguarded, alternated
        import time
        from music_amd.guard import GradGuard
        n = eng.spec.total
        eng.loss_and_grad(x, target)
        gd = GradGuard(eng.flat.device, 1.0, True, (0.9, 0.999))
        m, v = torch.zeros_like(eng.flat), torch.zeros_like(eng.flat)
        p = eng.flat.clone()

        def timed(fn):
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.reps * 20):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return round(ev[0].elapsed_time(ev[1]) / (args.reps * 20) * 1e3, 2)
        res["guard_floats"] = n
        res["grad_guard_us"] = timed(lambda: gd.run(ptr(eng.flat_grad), n, 1.0))
        res["adam_guarded_us"] = timed(lambda: call("wn_adam_flat_guarded", ptr(p), ptr(eng.flat_grad), ptr(m), ptr(v), n, 1e-4, 0.9, 0.999,
                                                    1e-8, 1.0, gd.state_ptr(), st))
        res["adam_plain_us"] = timed(lambda: call("wn_adam_flat", ptr(p), ptr(eng.flat_grad), ptr(m), ptr(v), n, 1e-4, 0.9, 0.999, 1e-8,
                                                  0.1, 0.001, 1.0, st))
        steps = {"unguarded": [], "guarded": []}
        for rnd in range(6):                               # alternated, as tools/ab_vars.py does
            for label in ("unguarded", "guarded"):
                eng.adam_init(lr=1e-4, max_grad_norm=1.0 if label == "guarded" else None, skip_nonfinite=label == "guarded")
                for _ in range(3):
                    eng.loss_and_grad(x, target)
                    eng.adam_step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps * 4):
                    eng.loss_and_grad(x, target)
                    eng.adam_step()
                torch.cuda.synchronize()
                steps[label].append((time.perf_counter() - t0) / (args.reps * 4) * 1e3)
        for label, vals in steps.items():
            res["fused_step_%s_ms" % label] = round(float(np.median(vals)), 4)
            res["fused_step_%s_ms_all" % label] = [round(t, 4) for t in vals]
        res["guard_report"] = eng.guard_report()
    if args.what == "ema":
        # the EMA shadow update on config 2's flat buffer: wn_ema_flat plain and behind a guard's state block, by HIP events over
        # `reps` back-to-back calls; then the whole fused step with / without EMA, alternated; written to profiles/ema_kbench.json
        import time
        from music_amd.guard import GradGuard
        n = eng.spec.total
        eng.loss_and_grad(x, target)
        gd = GradGuard(eng.flat.device, 1.0, True, (0.9, 0.999))
        gd.run(ptr(eng.flat_grad), n, 1.0)
        shadow = eng.flat.clone()

        def timed(fn):
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.reps * 20):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return round(ev[0].elapsed_time(ev[1]) / (args.reps * 20) * 1e3, 2)
        res["ema_floats"] = n
        res["ema_plain_us"] = timed(lambda: call("wn_ema_flat", ptr(shadow), ptr(eng.flat), n, 0.9999, 1, 1000, None, st))
        res["ema_guarded_us"] = timed(lambda: call("wn_ema_flat", ptr(shadow), ptr(eng.flat), n, 0.9999, 1, 0, gd.state_ptr(), st))
        steps = {"without_ema": [], "with_ema": []}
        for rnd in range(6):                               # alternated, as the guard leg does
            for label in ("without_ema", "with_ema"):
                eng.adam_init(lr=1e-4, ema_decay=0.9999 if label == "with_ema" else None, ema_warmup=True)
                for _ in range(3):
                    eng.loss_and_grad(x, target)
                    eng.adam_step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps * 4):
                    eng.loss_and_grad(x, target)
                    eng.adam_step()
                torch.cuda.synchronize()
                steps[label].append((time.perf_counter() - t0) / (args.reps * 4) * 1e3)
        for label, vals in steps.items():
            res["fused_step_%s_ms" % label] = round(float(np.median(vals)), 4)
            res["fused_step_%s_ms_all" % label] = [round(t, 4) for t in vals]
        res["fused_step_ema_delta_ms"] = round(res["fused_step_with_ema_ms"] - res["fused_step_without_ema_ms"], 4)
        res["fused_step_spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in steps.items()}
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "ema_kbench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if args.what == "nll":
        # the per-timestep softmax + NLL kernel (wn_step_nll) against the chunk softmax + CE kernel of the reference's loss
        # (wn_chunk_softmax256_ce) on config 2's logits (8 x 256 x 12930), alternated on one box, by HIP events over `reps * 20`
        # back-to-back calls; both read the logits once and write d loss / d logits once (2 B Q W 4 bytes).  Then the whole fused
        # step under both objectives, alternated.  Written to profiles/nll_kbench.json
        import time
        eng.loss_and_grad(x, target)
        bw = ws["bwd"]
        B, W, Q = B_LOCAL, ws["W"], eng.Q
        n = B * W
        part = ws["loss_part"]
        row_nll = torch.empty(n, dtype=torch.float32, device="cuda")
        row_hit = torch.empty(n, dtype=torch.int32, device="cuda")

        def timed(fn):
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.reps * 20):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / (args.reps * 20) * 1e3
        legs = {
            "chunk_softmax256_ce": lambda: call("wn_chunk_softmax256_ce", ptr(ws["O"]), ptr(target), None, ptr(bw["dO"]), ptr(part), n,
                                                1.0 / n, st),
            "step_nll": lambda: call("wn_step_nll", ptr(ws["O"]), Q * W, W, ptr(target), ptr(bw["dO"]), Q * W, W, None, None, None,
                                     ptr(part), W, Q, B, 1.0 / n, st),
            "step_nll_score": lambda: call("wn_step_nll", ptr(ws["O"]), Q * W, W, ptr(target), None, 0, 0, None, ptr(row_nll),
                                           ptr(row_hit), ptr(part), W, Q, B, 1.0 / n, st),
        }
        us = {k: [] for k in legs}
        for rnd in range(6):
            for k, fn in legs.items():
                us[k].append(timed(fn))
        nbytes = 2 * B * Q * W * 4
        res["nll_shape"] = [B, Q, W]
        res["nll_algorithmic_bytes"] = nbytes
        for k, vals in us.items():
            res[k + "_us"] = round(float(np.median(vals)), 2)
            res[k + "_us_all"] = [round(v, 2) for v in vals]
        res["step_nll_over_chunk_ce"] = round(res["step_nll_us"] / res["chunk_softmax256_ce_us"], 3)
        for k in ("chunk_softmax256_ce", "step_nll"):
            res[k + "_TBps"] = round(nbytes / (res[k + "_us"] * 1e-6) / 1e12, 3)
            res[k + "_share_of_8TBps"] = round(res[k + "_TBps"] / 8.0, 3)
        steps = {"reference": [], "nll": []}
        eng.adam_init(lr=1e-4)
        for rnd in range(6):                               # alternated, as the guard and ema legs do
            for label in steps:
                for _ in range(3):
                    eng.loss_and_grad(x, target, objective=label)
                    eng.adam_step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps * 4):
                    eng.loss_and_grad(x, target, objective=label)
                    eng.adam_step()
                torch.cuda.synchronize()
                steps[label].append((time.perf_counter() - t0) / (args.reps * 4) * 1e3)
        for label, vals in steps.items():
            res["fused_step_%s_ms" % label] = round(float(np.median(vals)), 4)
            res["fused_step_%s_ms_all" % label] = [round(t, 4) for t in vals]
        res["fused_step_nll_delta_ms"] = round(res["fused_step_nll_ms"] - res["fused_step_reference_ms"], 4)
        res["fused_step_spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in steps.items()}
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "nll_kbench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if args.what == "cond":
        # the learned conditioning projections (wn_cond_proj_fwd: one launch; wn_cond_proj_bwd: two) alone at config 4's shape and at
        # the shipped autoencoder's, by HIP events over `reps * 20` back-to-back calls, six alternations; then the fused config-4
        # step with conditioning="learned" against "random" on one box, alternated.  Written to profiles/cond_kbench.json
        import time
        from music_amd.model1 import wavenet_autoencoder

        def timed(fn):
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.reps * 20):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / (args.reps * 20) * 1e3
        shapes = {"config4": dict(N=30, Dd=64, CH=64, Sd=256, Bw=64, Le=25, B=8, pair=False),
                  "shipped": dict(N=40, Dd=32, CH=32, Sd=512, Bw=512, Le=32, B=4, pair=True)}
        for tag, g in shapes.items():
            N, Dd, CH, Sd, Bw, Le, B, pair = (g[k] for k in ("N", "Dd", "CH", "Sd", "Bw", "Le", "B", "pair"))
            rnd = lambda *shape: torch.randn(*shape, device="cuda")
            stride = 2 * Dd * Bw + 2 * Dd
            n = N * stride + Sd * Bw + Sd
            flat, grad, enc = rnd(n) * 0.1, torch.empty(n, device="cuda"), rnd(B, Bw, Le)
            offs = (0, 2 * Dd * Bw, stride, N * stride, N * stride + Sd * Bw)
            dims = (N, Dd, CH, Sd, Bw, Le, B)
            tab, tabp, enf = rnd(N, B, 2 * CH, Le), (rnd(N, B // 2, 4 * CH, Le) if pair else None), rnd(B, Sd, Le)
            d_enc = torch.empty(B, Bw, Le, device="cuda")
            legs = {"fwd": lambda: call("wn_cond_proj_fwd", ptr(enc), ptr(flat), *offs, ptr(tab), ptr(tabp), ptr(enf), *dims, st),
                    "bwd": lambda: call("wn_cond_proj_bwd", ptr(tabp if pair else tab), 1 if pair else 0, ptr(enf), ptr(enc), ptr(flat), *offs,
                                        ptr(d_enc), ptr(grad), *dims, st)}
            us = {k: [] for k in legs}
            for _ in range(6):
                for k, fn in legs.items():
                    us[k].append(timed(fn))
            R, C = N * 2 * Dd + Sd, B * Le
            res["cond_%s_shape" % tag] = g
            res["cond_%s_flop" % tag] = {"fwd": 2 * R * C * Bw, "bwd": 4 * R * C * Bw}
            for k, vals in us.items():
                res["cond_%s_%s_us" % (tag, k)] = round(float(np.median(vals)), 2)
                res["cond_%s_%s_us_all" % (tag, k)] = [round(v, 2) for v in vals]
        steps, engines = {"random": [], "learned": []}, {}
        for label in steps:
            torch.manual_seed(0)
            ae = wavenet_autoencoder(filter_width=2, quantization_channel=256, dilations=CFG["dilations"], en_residual_channel=64,
                                     en_dilation_channel=64, en_bottleneck_width=64, en_pool_kernel_size=512, de_residual_channel=64,
                                     de_dilation_channel=64, de_skip_channel=256, use_bias=False, conditioning=label).cuda()
            engines[label] = (ae, ae._engine_for(x.device))
            engines[label][1].adam_init(lr=1e-4)

        def fused(label):
            ae, aeng = engines[label]
            aeng.loss_and_grad(x, target, ae.engine_cond())
            aeng.adam_step()
        for rnd_ in range(6):
            for label in steps:
                for _ in range(3):
                    fused(label)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps * 4):
                    fused(label)
                torch.cuda.synchronize()
                steps[label].append((time.perf_counter() - t0) / (args.reps * 4) * 1e3)
        for label, vals in steps.items():
            res["fused_c4_step_%s_ms" % label] = round(float(np.median(vals)), 4)
            res["fused_c4_step_%s_ms_all" % label] = [round(t, 4) for t in vals]
        res["fused_c4_step_learned_delta_ms"] = round(res["fused_c4_step_learned_ms"] - res["fused_c4_step_random_ms"], 4)
        res["fused_c4_step_spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in steps.items()}
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "cond_kbench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if args.what in ("ae", "all"):
        # BASELINE config 4: autoencoder, 30+30 blocks, 64 ch, skip 256, bottleneck 64, pool 512, batch 8 x 16000:
        # forward + CE + backward (fresh conditioning projections every forward, as in the reference)
        import time
        from music_amd.model1 import wavenet_autoencoder
        torch.manual_seed(0)
        ae = wavenet_autoencoder(filter_width=2, quantization_channel=256, dilations=CFG["dilations"], en_residual_channel=64,
                                 en_dilation_channel=64, en_bottleneck_width=64, en_pool_kernel_size=512,
                                 de_residual_channel=64, de_dilation_channel=64, de_skip_channel=256, use_bias=False).cuda()
        opt = torch.optim.Adam(ae.parameters(), lr=1e-4)
        lossf = torch.nn.CrossEntropyLoss()

        def ae_step():
            opt.zero_grad()
            loss = lossf(ae(x), target)
            loss.backward()
            opt.step()
            return loss
        for _ in range(2):
            ae_step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            loss = ae_step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        res["autoencoder_step_ms"] = round(dt * 1e3, 2)
        res["autoencoder_samples_per_s"] = round(B_LOCAL * T / dt, 1)
        res["autoencoder_loss"] = round(float(loss.item()), 5)
        # the fused step of the engine (one softmax + CE + backward kernel, flat Adam; no autograd, no per-tensor optimizer)
        aeng = ae._engine_for(x.device)
        aeng.adam_init(lr=1e-4)

        def ae_fused():
            loss = aeng.loss_and_grad(x, target, ae._draw_conditioning())
            aeng.adam_step()
            return loss
        for _ in range(2):
            ae_fused()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            loss = ae_fused()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        res["autoencoder_fused_step_ms"] = round(dt * 1e3, 2)
        res["autoencoder_fused_samples_per_s"] = round(B_LOCAL * T / dt, 1)
        # cached-queue generation from the autoencoder (one pooled frame of encoding, conditioning folded into biases)
        from music_amd import ae_generate as ag
        piece = torch.zeros(1, 256, ae.receptive_field + 512, device="cuda")
        piece[:, 128, :] = 1.0
        try:
            ag.generate_cached(ae, piece, 200)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ag.generate_cached(ae, piece, 8000)
            torch.cuda.synchronize()
            res["autoencoder_cached_generation_samples_per_s"] = round(8000 / (time.perf_counter() - t0), 1)
        except ValueError as e:           # (the piece must pool to exactly one frame)
            res["autoencoder_cached_generation"] = str(e)[:120]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
