#!/usr/bin/env python3
"""Developer tool (GPU): cached-queue decode speed of the config-5 model (30 blocks, 64 / 64 / 256 / 256), one stream and
batches, as bench.py's extra.c5_decode measures it; honours the WN_DEC_* switches.  `--bias`: a biased model (the
autoencoder's cached decoder is one).  `--filter-width K`: the same shape with K taps (K != 2 runs the corrected queue
recurrence, the only one defined there).  `--cond-frames N`: the same decoder CONDITIONED (wn_decode_batch_cond) on per-utterance
tables of N frames with the schedule of a 16000-sample clip (config 4: N = 25), biased, corrected recurrence, from zero queues -
to be compared with `--bias` (the unconditioned biased decoder of the same shape).
`--temperature T`: sample instead of the greedy argmax; `--top-k K` / `--top-p P`: truncate the distribution first
(wn_decode_batch_samp; corrected recurrence, temperature 1 unless given); `--windows S,K`: sample under the position windows of an
S-stage token stream of K codes per stage (wn_win_decode_batch with fast_generate.stage_windows(S, K); corrected recurrence,
temperature 1 unless given); `--runs N`: repeat the whole measurement.
`--keep S,n`: partially forced decode over the default shape - a stage-prefix mask, positions with p % S < n are kept (fed a fixed
token), the others drawn (generate_codes(keep=): one launch; corrected recurrence, temperature 1 unless given) - to be compared with
`--temperature 1 --corrected` (the free run of the same build on the same recurrence); `--corrected`: the corrected recurrence.
`--guidance S`: classifier-free guidance at scale S (wn_cfg_decode_batch) on the class-conditional model of the same shape, and on a
code prior's shape (10 blocks, 64 / 64 / 256, Q = 1024: the fp32 kernel, two members per workgroup, under stage windows 4 x 256):
U guided streams against 2 U plain conditioned rows of the same build, U = 1 and 64, alternated six times, medians; `--json PATH`
writes the figures."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def filter_width():
    return int(sys.argv[sys.argv.index("--filter-width") + 1]) if "--filter-width" in sys.argv else 2


def cond_frames():
    return int(sys.argv[sys.argv.index("--cond-frames") + 1]) if "--cond-frames" in sys.argv else 0


def _opt(name, conv, default=None):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def sampling():
    """generate_codes' sampling arguments from the command line, and whether they need the corrected recurrence"""
    top_k, top_p = _opt("--top-k", int), _opt("--top-p", float)
    windows = _opt("--windows", lambda v: tuple(int(x) for x in v.split(",")))
    filtered = top_k is not None or top_p is not None
    T = _opt("--temperature", float, 1.0 if filtered or windows or "--keep" in sys.argv else None)
    kw = dict(temperature=T, seed=1)
    if filtered:
        kw.update(top_k=top_k, top_p=top_p)
    if windows:
        from music_amd import fast_generate as fg
        kw.update(windows=fg.stage_windows(*windows))
    return kw, filtered or bool(windows) or "--keep" in sys.argv or "--corrected" in sys.argv


def keep_mask(U, n):
    """`--keep S,n` as generate_codes' keyword: (U, n) tokens - position p holds (128 + p) % 256 where p % S < n, -1 elsewhere"""
    sn = _opt("--keep", lambda v: tuple(int(x) for x in v.split(",")))
    if sn is None:
        return {}
    p = torch.arange(n)
    return {"keep": torch.where(p % sn[0] < sn[1], (128 + p) % 256, torch.full_like(p, -1)).repeat(U, 1)}


def main_cond(le):
    """conditioned decode of the config-4 decoder shape: one stream x 12930 positions, 128 utterances x 2000"""
    from music_amd import ae_generate as ag
    from music_amd import fast_generate as fg
    from music_amd.model import wavenet
    torch.manual_seed(0)
    cfg = dict(bench.CFG, use_bias=True, filter_width=2)
    net = wavenet(**cfg).cuda()
    dev = torch.device("cuda", 0)
    eng = net._engine_for(dev)
    N, rf = len(cfg["dilations"]), net.receptive_field
    W = 16000 - rf + 1
    sched = ag.cond_schedule((2, cfg["dilations"]), W, le)
    rw = fg._ring_width(eng)
    for U, n in ((1, W), (128, 2000)):
        tabs = dict(cond_fg=0.1 * torch.randn(U, N, le, 2 * 64, device=dev), cond_p1=0.1 * torch.randn(U, le, cfg["skip_channels"], device=dev),
                    schedule=sched)
        note = torch.zeros(U, 256, device=dev)
        note[torch.arange(U), (128 + torch.arange(U)) % 256] = 1.0
        for rep in range(3):
            rings = torch.zeros(U, sum(d * rw for d in eng.dil), device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            codes, _, _, _ = fg.decode_batch_cond(net, rings, note.clone().view(U, 1, 256), note, n, step0=0, pos0=0, **tabs)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("conditioned (%d frames), %d utterance(s) x %d samples, run %d: %.3f s = %.1f k samples/s (%d distinct codes)"
                  % (le, U, n, rep, dt, U * n / dt / 1e3, int(torch.unique(codes).numel())))


def main_guided(scale):
    """U guided streams (2 U rows, one choice per pair) against 2 U plain conditioned rows: what guidance costs beyond its second row"""
    from music_amd import fast_generate as fg
    from music_amd.model import wavenet
    dev = torch.device("cuda", 0)
    gl = dict(global_classes=4, global_channels=16, null_class=3)
    shapes = [("config-5 shape (matrix cores)", dict(bench.CFG, use_bias=False, filter_width=2, **gl), None, 16000, 2000),
              ("prior shape, Q = 1024 (fp32 kernel)", dict(filter_width=2, dilations=[2 ** i for i in range(10)], dilation_channels=64,
                                                        residual_channels=64, skip_channels=256, quantization_channels=1024,
                                                        use_bias=False, **gl), fg.stage_windows(4, 256), 2000, 500)]
    res = {"what": "guided streams against twice as many plain conditioned rows, k samples/s of ROWS (a guided stream counts as two), "
                   "6 alternations, medians [min, max]", "guidance": scale, "cases": []}
    for name, cfg, win, n1, n64 in shapes:
        torch.manual_seed(0)
        net = wavenet(**cfg).cuda()
        Q = cfg["quantization_channels"]
        for U, n in ((1, n1), (64, n64)):
            def pieces(rows):
                st = torch.zeros(rows, Q, net.receptive_field, device=dev)
                st[torch.arange(rows), (Q // 2 + torch.arange(rows)) % Q, :] = 1.0
                return st
            kw = dict(correct_queue=True, temperature=1.0, seed=1, windows=win)
            runs = {"guided": lambda: fg.generate_codes_batch(net, pieces(U), n + 1, classes=[u % 3 for u in range(U)], guidance=scale, **kw),
                    "plain": lambda: fg.generate_codes_batch(net, pieces(2 * U), n + 1, classes=[u % 3 for u in range(2 * U)], **kw)}
            t = {"guided": [], "plain": []}
            for alt in range(7):                            # (the first alternation warms up: not counted)
                for key in ("guided", "plain"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    runs[key]()
                    torch.cuda.synchronize()
                    if alt:
                        t[key].append(2 * U * n / (time.perf_counter() - t0) / 1e3)
            row = {"shape": name, "streams": U, "rows": 2 * U, "steps": n}
            for key in t:
                row[key] = {"median": statistics.median(t[key]), "min": min(t[key]), "max": max(t[key])}
            row["guided_over_plain"] = row["guided"]["median"] / row["plain"]["median"]
            res["cases"].append(row)
            print("%s, %d guided stream(s) against %d plain rows x %d samples: %.1f [%.1f, %.1f] against %.1f [%.1f, %.1f] k row-samples/s = %.3fx"
                  % (name, U, 2 * U, n, row["guided"]["median"], row["guided"]["min"], row["guided"]["max"], row["plain"]["median"],
                     row["plain"]["min"], row["plain"]["max"], row["guided_over_plain"]))
    path = _opt("--json", str)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


def main():
    if cond_frames():
        return main_cond(cond_frames())
    if "--guidance" in sys.argv:
        return main_guided(_opt("--guidance", float))
    from music_amd import fast_generate as fg
    from music_amd.model import wavenet
    torch.manual_seed(0)
    k = filter_width()
    cfg = dict(bench.CFG, use_bias="--bias" in sys.argv, filter_width=k)
    net = wavenet(**cfg).cuda()
    dev = torch.device("cuda", 0)
    start = torch.zeros(1, 256, net.receptive_field, device=dev)
    start[0, 128, :] = 1.0
    n = 16000
    kw, filtered = sampling()
    correct = k != 2 or filtered
    what = ", ".join("%s %s" % (key, "%d pairs" % len(v) if key == "windows" else v) for key, v in kw.items()
                     if v is not None and key != "seed") or "greedy"
    if "--keep" in sys.argv:
        what += ", keep %s" % _opt("--keep", str)
    for run in range(_opt("--runs", int, 1)):
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seq = fg.generate_codes(net, start, n, correct_queue=correct, **kw, **keep_mask(1, n))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        print("one stream (%s): %d samples in %.3f s = %.1f k samples/s = %.2f us per sample (%d distinct codes)"
              % (what, n, dt, n / dt / 1e3, dt / n * 1e6, int(torch.unique(seq).numel())))
        for U in ((128, 1024) if fg._mfma_decode(net._engine) else (128,)):          # (the fp32 kernel: at most 128 per launch)
            st = torch.zeros(U, 256, net.receptive_field, device=dev)
            for uu in range(U):
                st[uu, (128 + uu) % 256, :] = 1.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fg.generate_codes_batch(net, st, 2001, correct_queue=correct, **kw, **keep_mask(U, 2001))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("%d utterances x 2000 samples (%s): %.3f s = %.2f M samples/s" % (U, what, dt, U * 2000 / dt / 1e6))


if __name__ == "__main__":
    main()
