"""Window decode against today's composite (profiles/r05_window_decode.txt).

Corpus: --streams stereo 4-bit streams of --seconds s at 48 kHz resident on the device as .aad images, synthesised from a seed
(aad_amd/synth.py) and encoded on the device with a segmented plan (the images' bytes do not matter to a decode, only their layout).
Windows: N random (stream, first_frame) pairs drawn on the device, T frames each; one table per N, the same for every row.

Rows (kernel times from the events of AADHip_ContextSignalNextRun, median of --reps; call times wall clock with a device synchronise):
  (a) the existing decoder over the same covering blocks as a bare-block plan (AADHip_DecodePlanRun, has_file_header = 0, one table
      entry per block), int16 interleaved: the "auto" policy's choice and "dense" - kernel only, the plan made beforehand;
  (b) today's composite per call: covering-block table on the host from the windows (.cpu()), plan create + upload, bare-block decode,
      torch gather + transpose to [N, C, T], .float() / 32768;
  (c) the window run (AADHip_WindowDecodePlanRun), int16 and float32: kernel and call.
Bit-exact: (a) auto == (a) dense; every crop of (b) and (c) == the crop gathered from (a) dense, float32 == int16 / 32768 bitwise;
and a few windows against the oracle's decode of the whole stream (tests/oracle_binding.py, when present).

--mixed (profiles/r06_window_decode_mixed.txt): the mixed-format plan (AADHip_MixedWindowDecodePlanCreate), float32 rows.
  (a) a one-variant mixed plan against the same-format plan over the same images and windows; the same-format plan is timed twice
      first, and the difference of its two medians is the tool's own run-to-run spread;
  (b) a corpus of one third each 2-, 3- and 4-bit stereo streams: the mixed plan's run (three kernels) against today's composite -
      the window table to the host, split by format, one same-format run per format over its own table, the rows scattered into
      [N, C, T] (the three plans made beforehand).  Every row of the mixed run is compared with the composite's.

--channel-mix (profiles/r07_window_decode_channel_mix.txt): the channel-mix plan (AADHip_ChannelMixWindowDecodePlanCreate) down to
one float32 row per window, on an all-stereo corpus and on one whose every second stream is mono (4-bit, the tool's shapes):
  (a) the channel-mix plan with out_channels = 1: call time, and first kernel start to last kernel stop;
  (b) what a caller has without it.  All stereo: the mixed-format plan into [N, 2, T], then (y[:, 0] + y[:, 1]) * 0.5 in torch.
      Half mono: the mixed-format plan refuses the corpus, so the window table goes to the host and is split by channel count, a
      mono and a stereo mixed-format plan (made beforehand) run over their own tables, the stereo rows are mixed in torch and both
      parts scattered into [N, 1, T].
  Both are warmed up, then timed in alternating rounds of --reps calls; a figure is the median of the rounds' medians and its spread
  the range of the rounds' medians.  Every row of (a) is compared with (b)'s bitwise.

--stats (profiles/r08_window_decode_stats.txt): the level statistics of the rows (AADHip_WindowDecodePlanRunStats) on the tool's
corpus - stereo 4-bit, float32 rows, same-format plan:
  (a) AADHip_WindowDecodePlanRun alone;
  (b) rows and the statistics table in one run;
  (c) the table alone (device_out = NULL: nothing is stored but the records);
  (d) what a caller has without it: (a), then y.square().sum(-1), y.abs().sum(-1) and y.abs().amax(-1) over the float32 rows.
  All four are warmed up, then timed in alternating rounds of --reps calls (wall clock with a device synchronise); a figure is
  the median of the rounds' medians and its spread the range of the rounds' medians.  (b)'s rows are compared with (a)'s bitwise,
  (b)'s table with (c)'s, and the table with int64 sums over the int16 rows taken in torch.

--half (profiles/window_decode_half.txt): the run's kernel per sample type - int16, float32, float16 and bfloat16, those the
loaded library has (AAD_HIP_LIBRARY names another build, e.g. the parent commit's, which refuses the last two) - on the tool's
corpus, same-format plan.  Kernel times from the events of AADHip_ContextSignalNextRun: per type the median of --reps, in
alternating rounds over the types; a figure is the median of the rounds' medians and its spread the range of the rounds' medians.
float16 and bfloat16 rows are compared bitwise with torch's conversion of the float32 rows.

--gain (profiles/window_decode_gain.txt): the gain run (AADHip_WindowDecodePlanRunGain) on the tool's corpus - stereo 4-bit,
float32 rows, same-format plan, two window tables (a "signal" and a "noise" draw) and two float32 [N] gain tables:
  (a) AADHip_WindowDecodePlanRun alone;
  (b) a STORE run: gs * x;
  (c) an ADD run: gn * y added into rows that are there;
  (d) what a caller has without it: two plain runs, then gs[:, None, None] * x + gn[:, None, None] * y in torch - against
      (b) followed by (c) into one buffer, "(b)+(c)".
  All are warmed up, then timed in alternating rounds of --reps calls (wall clock with a device synchronise); a figure is the
  median of the rounds' medians and its spread the range of the rounds' medians.  (b)+(c)'s rows are compared bitwise with torch's
  two-rounding expression x * gs + y * gn over the plain rows ((d)'s own expression may be contracted differently by torch).

--placed (profiles/window_decode_placed.txt): the run with a span per window (AADHip_WindowDecodePlanRunPlaced) on --gain's
corpus, float32 rows, same-format plan, one window table, one gain table:
  (a) AADHip_WindowDecodePlanRunGain, STORE;
  (b) the placed run, STORE, every span (T, 0);
  (c) the placed run, STORE, L = T / 2 at a random o in [0, T - L];
  (d) the placed run, ADD, L = T / 4 at a random o in [0, T - L], into rows that are there;
  (e) what (d) replaces: a plain run with T' = T / 4 into a temporary, then out[w, :, o:o+L] += g[w] * tmp[w] for all windows in
      one torch scatter-add over an index tensor (a loop over the distinct offsets would be N small kernels).
  Warm-up, alternating rounds and the figures as under --gain.  (b)'s rows are compared bitwise with (a)'s, (c)'s and (d)'s with
  torch's expression of the definition over the plain rows.

Usage: python tools/window_decode_bench.py [--streams 1000] [--seconds 60] [--windows 4096 64] [--frames 48000] [--reps 25]
       [--mixed | --channel-mix | --stats | --half | --gain | --placed]"""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 8.0e12


def build_corpus(engine, torch, streams, samples, chunk=25, seed=11, bits=4, channels=2):
    from aad_amd.capi import make_parameter
    from aad_amd.synth import synth_pcm
    param = make_parameter(channels, bits, 1024)
    size = engine.encoded_size(param, samples)
    stride = (size + 63) // 64 * 64
    corpus = torch.zeros((streams, stride), dtype=torch.uint8, device="cuda")
    starts = list(range(0, streams, chunk))
    gen = lambda s0: synth_pcm(min(chunk, streams - s0), samples, channels, seed=seed, first_stream=s0)
    with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for s0, pcm in zip(starts, pool.map(gen, starts)):
            img, got = engine.encode_uniform(torch.from_numpy(pcm).cuda(), param, segment_blocks=16, warmup_blocks=1)
            assert got == size
            corpus[s0:s0 + img.shape[0], :] = img[:, :stride]
            del img
    torch.cuda.synchronize()
    return corpus, size, stride


def covering_blocks(win, frames, spb, bs, size, samples, stride):
    """host table of the blocks that cover each window (one bare-block stream each) and where each window's crop starts in
    the decoded frames"""
    s, f = win[:, 0].astype(np.uint64), win[:, 1].astype(np.uint64)
    b0, b1 = f // spb, (f + frames - 1) // spb
    count = (b1 - b0 + 1).astype(np.int64)
    total = int(count.sum())
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    w_of = np.repeat(np.arange(len(win)), count)
    blk = b0[w_of] + (np.arange(total) - first[w_of]).astype(np.uint64)
    from aad_amd.capi import STREAM_DESC_DTYPE
    t = np.zeros(total, dtype=STREAM_DESC_DTYPE)
    t["data_offset"] = s[w_of] * np.uint64(stride) + np.uint64(31) + blk * np.uint64(bs)
    t["data_size"] = np.minimum(np.uint64(bs), np.uint64(size - 31) - blk * np.uint64(bs))
    t["num_samples"] = np.minimum(np.uint64(spb), np.uint64(samples) - blk * np.uint64(spb))
    t["pcm_offset"] = np.arange(total, dtype=np.uint64) * np.uint64(spb * 2)
    crop0 = first.astype(np.int64) * spb + (f % np.uint64(spb)).astype(np.int64)  # frame of each crop in the decoded blocks
    return t, crop0


def kernel_ms(engine, HipEvent, fn, reps):
    out = []
    for _ in range(reps):
        start, stop = HipEvent(timing=True), HipEvent(timing=True)
        engine.signal_next(stop, start=start)
        fn()
        stop.synchronize()
        out.append(start.elapsed_ms(stop))
        start.close()
        stop.close()
    return float(np.median(out))


def call_ms(torch, fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def gather(torch, pcm_blocks, crop0, frames):
    """decoded interleaved frames [frames_total, 2] -> [N, 2, T] int16"""
    idx = torch.as_tensor(crop0, device="cuda")[:, None] + torch.arange(frames, device="cuda")[None, :]
    return pcm_blocks.view(-1, 2)[idx].transpose(1, 2).contiguous()


def mixed_main(args, say):
    import torch
    from aad_amd.capi import STREAM_DESC_DTYPE
    from aad_amd.engine import Engine, HipEvent, parse_header
    engine = Engine(0)
    samples, frames, streams = int(round(args.seconds * 48000)), args.frames, args.streams
    results = []

    def uniform_table(count, stride, size):
        d = np.zeros(count, dtype=STREAM_DESC_DTYPE)
        d["data_offset"] = np.arange(count, dtype=np.uint64) * np.uint64(stride)
        d["data_size"], d["num_samples"] = size, samples
        return d

    def draw(n, count):
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed + n)
        return torch.stack([torch.randint(0, count, (n,), device="cuda", generator=g),
                            torch.randint(0, samples - frames + 1, (n,), device="cuda", generator=g)], dim=1)

    # (a) one variant: the same images and windows under both plans
    corpus, size, stride = build_corpus(engine, torch, streams, samples, seed=args.seed)
    hd = parse_header(bytes(corpus[0, :31].cpu().numpy()))
    say("mixed window decode (a): %d stereo 4-bit streams x %d frames, T = %d, float32 rows, median of %d; device %s"
        % (streams, samples, frames, args.reps, torch.cuda.get_device_name(0)))
    same = engine.uniform_window_decode_plan(hd, streams, stride, size)
    mixed = engine.mixed_window_decode_plan([hd] * streams, uniform_table(streams, stride, size), True)
    for n in args.windows:
        d_win = draw(n, streams)
        out_s = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        out_m = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        s1 = kernel_ms(engine, HipEvent, lambda: same.run(corpus, d_win, frames, torch.float32, out=out_s), args.reps)
        s2 = kernel_ms(engine, HipEvent, lambda: same.run(corpus, d_win, frames, torch.float32, out=out_s), args.reps)
        m = kernel_ms(engine, HipEvent, lambda: mixed.run(corpus, d_win, frames, torch.float32, out=out_m), args.reps)
        s3 = kernel_ms(engine, HipEvent, lambda: same.run(corpus, d_win, frames, torch.float32, out=out_s), args.reps)
        torch.cuda.synchronize()
        exact = bool(torch.equal(out_s.view(torch.int32), out_m.view(torch.int32)))
        spread, base = abs(s1 - s2), min(s1, s2)
        say("  N = %5d: same-format kernel %.4f / %.4f ms (spread %.4f; again after the mixed run: %.4f), one-variant mixed kernel "
            "%.4f ms: %+.4f ms = %+.2f %% (more than twice the spread: %s); identical rows: %s"
            % (n, s1, s2, spread, s3, m, m - base, 100 * (m - base) / base, m - base > 2 * spread, exact))
        results.append(dict(part="a", windows=n, same_ms=[s1, s2, s3], mixed_ms=m, identical=exact))
        del out_s, out_m
    same.close()
    mixed.close()
    del corpus
    torch.cuda.empty_cache()

    # (b) three variants: one third each of 2-, 3- and 4-bit streams (stream i has bits (2, 3, 4)[i % 3])
    third = streams // 3
    parts = {b: build_corpus(engine, torch, third, samples, seed=args.seed + b, bits=b) for b in (2, 3, 4)}
    stride = max(p[2] for p in parts.values())
    corpus = torch.zeros((3 * third, stride), dtype=torch.uint8, device="cuda")
    table = np.zeros(3 * third, dtype=STREAM_DESC_DTYPE)
    table["data_offset"] = np.arange(3 * third, dtype=np.uint64) * np.uint64(stride)
    table["num_samples"] = samples
    headers, plans = [None] * (3 * third), {}
    for j, b in enumerate((2, 3, 4)):
        img, size_b, stride_b = parts[b]
        corpus[j::3, :stride_b] = img
        table["data_size"][j::3] = size_b
        h = parse_header(bytes(img[0, :31].cpu().numpy()))
        headers[j::3] = [h] * third
        plans[j] = engine.window_decode_plan(h, table[j::3], True)  # the format's own streams: stream s of the corpus is s // 3 here
    del parts
    mixed = engine.mixed_window_decode_plan(headers, table, True)
    say("")
    say("mixed window decode (b): %d streams, one third each 2-, 3- and 4-bit stereo (spb %s), T = %d, float32 rows"
        % (3 * third, "/".join(str(headers[j].num_samples_per_block) for j in range(3)), frames))
    for n in args.windows:
        d_win = draw(n, 3 * third)
        out_m = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        out_c = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")

        def composite():
            w = d_win.cpu()  # the host synchronisation the mixed plan removes
            for j in range(3):
                idx = torch.nonzero(w[:, 0] % 3 == j).flatten()
                sub = torch.stack([w[idx, 0] // 3, w[idx, 1]], dim=1).cuda()
                out_c[idx.cuda()] = plans[j].run(corpus, sub, frames, torch.float32)

        km = kernel_ms(engine, HipEvent, lambda: mixed.run(corpus, d_win, frames, torch.float32, out=out_m), args.reps)
        cm = call_ms(torch, lambda: mixed.run(corpus, d_win, frames, torch.float32, out=out_m), args.reps)
        cc = call_ms(torch, composite, args.reps)
        torch.cuda.synchronize()
        exact = bool(torch.equal(out_m.view(torch.int32), out_c.view(torch.int32)))
        say("  N = %5d: mixed plan, three kernels: first start to last stop %.4f ms, call %.4f ms; composite (three runs over "
            "host-split tables + scatter) call %.4f ms: %.2fx; identical rows: %s" % (n, km, cm, cc, cc / cm, exact))
        results.append(dict(part="b", windows=n, mixed_kernels_ms=km, mixed_call_ms=cm, composite_call_ms=cc, identical=exact))
        del out_m, out_c
    say("")
    say("json " + json.dumps(results))
    mixed.close()
    for p in plans.values():
        p.close()
    engine.close()


def channel_mix_main(args, say):
    import torch
    from aad_amd.capi import STREAM_DESC_DTYPE
    from aad_amd.engine import Engine, HipEvent, parse_header
    engine = Engine(0)
    samples, frames, streams = int(round(args.seconds * 48000)), args.frames, args.streams
    rounds, results = 5, []

    def draw(n, count):
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed + n)
        return torch.stack([torch.randint(0, count, (n,), device="cuda", generator=g),
                            torch.randint(0, samples - frames + 1, (n,), device="cuda", generator=g)], dim=1)

    def alternate(fa, fb):
        """warm both up, then rounds of (a), (b): per side the median of the rounds' medians and their range"""
        for _ in range(3):
            fa()
            fb()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(call_ms(torch, fa, args.reps))
            tb.append(call_ms(torch, fb, args.reps))
        return (float(np.median(ta)), max(ta) - min(ta)), (float(np.median(tb)), max(tb) - min(tb))

    say("channel-mix window decode to one float32 row per window: %d 4-bit streams x %d frames, T = %d; %d alternating rounds of %d "
        "calls, median of the rounds' medians (range of the rounds' medians); device %s"
        % (streams, samples, frames, rounds, args.reps, torch.cuda.get_device_name(0)))
    for name in ("all stereo", "half mono"):
        half = streams // 2
        stereo, size2, stride2 = build_corpus(engine, torch, streams if name == "all stereo" else half, samples, seed=args.seed)
        h2 = parse_header(bytes(stereo[0, :31].cpu().numpy()))
        if name == "all stereo":
            count, corpus, stride = streams, stereo, stride2
            headers, sizes = [h2] * count, np.full(count, size2, dtype=np.uint64)
        else:  # stream i is mono for even i, stereo for odd i
            mono, size1, stride1 = build_corpus(engine, torch, half, samples, seed=args.seed + 1, channels=1)
            h1 = parse_header(bytes(mono[0, :31].cpu().numpy()))
            count, stride = 2 * half, max(stride1, stride2)
            corpus = torch.zeros((count, stride), dtype=torch.uint8, device="cuda")
            corpus[0::2, :stride1] = mono
            corpus[1::2, :stride2] = stereo
            headers, sizes = [h1, h2] * half, np.array([size1, size2] * half, dtype=np.uint64)
            del mono
        del stereo
        table = np.zeros(count, dtype=STREAM_DESC_DTYPE)
        table["data_offset"] = np.arange(count, dtype=np.uint64) * np.uint64(stride)
        table["data_size"], table["num_samples"] = sizes, samples
        mix = engine.channel_mix_window_decode_plan(headers, table, 1, True)
        if name == "all stereo":
            plans = {2: engine.mixed_window_decode_plan(headers, table, True)}
        else:  # the channel count's own streams: stream s of the corpus is s // 2 there
            plans = {1: engine.mixed_window_decode_plan(headers[0::2], table[0::2], True),
                     2: engine.mixed_window_decode_plan(headers[1::2], table[1::2], True)}
        say("")
        say("%s: %d streams (%s), %.2f GB of images" % (name, count, "spb %d" % h2.num_samples_per_block if name == "all stereo" else
                                                         "mono spb %d, stereo spb %d" % (h1.num_samples_per_block, h2.num_samples_per_block),
                                                         count * stride / 1e9))
        for n in args.windows:
            d_win = draw(n, count)
            out_a = torch.empty((n, 1, frames), dtype=torch.float32, device="cuda")
            out_b = torch.empty((n, 1, frames), dtype=torch.float32, device="cuda")
            wide = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")

            def new_plan():
                mix.run(corpus, d_win, frames, torch.float32, out=out_a)

            def parent_stereo():
                y = plans[2].run(corpus, d_win, frames, torch.float32, out=wide)
                torch.mul(y[:, 0] + y[:, 1], 0.5, out=out_b[:, 0])

            def parent_half_mono():
                w = d_win.cpu()  # the host synchronisation the channel-mix plan removes
                for c in (1, 2):
                    idx = torch.nonzero(w[:, 0] % 2 == c - 1).flatten()
                    sub = torch.stack([w[idx, 0] // 2, w[idx, 1]], dim=1).cuda()
                    y = plans[c].run(corpus, sub, frames, torch.float32)
                    out_b[idx.cuda()] = y if c == 1 else ((y[:, 0] + y[:, 1]) * 0.5)[:, None]

            parent = parent_stereo if name == "all stereo" else parent_half_mono
            (a, a_range), (b, b_range) = alternate(new_plan, parent)
            ka = kernel_ms(engine, HipEvent, new_plan, args.reps)
            torch.cuda.synchronize()
            exact = bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)))
            say("  N = %5d: (a) channel-mix plan, out_channels = 1: call %.4f ms (range %.4f), kernels first start to last stop %.4f ms; "
                "(b) %s: call %.4f ms (range %.4f); (b) / (a) = %.2fx; (a) no slower than (b): %s; identical rows: %s"
                % (n, a, a_range, ka, "mixed-format plan into [N, 2, T] + torch mix" if name == "all stereo" else
                   "host split + two mixed-format plans + torch mix + scatter", b, b_range, b / a, a <= b, exact))
            results.append(dict(corpus=name, windows=n, a_call_ms=a, a_range_ms=a_range, a_kernels_ms=ka, b_call_ms=b, b_range_ms=b_range,
                                identical=exact))
            del out_a, out_b, wide
        mix.close()
        for p in plans.values():
            p.close()
        del corpus
        torch.cuda.empty_cache()
    say("")
    say("json " + json.dumps(results))
    engine.close()


def stats_main(args, say):
    import torch
    from aad_amd.engine import Engine, parse_header
    engine = Engine(0)
    samples, frames, streams = int(round(args.seconds * 48000)), args.frames, args.streams
    rounds, results = 5, []
    corpus, size, stride = build_corpus(engine, torch, streams, samples, seed=args.seed)
    hd = parse_header(bytes(corpus[0, :31].cpu().numpy()))
    plan = engine.uniform_window_decode_plan(hd, streams, stride, size)
    say("window decode statistics: %d stereo 4-bit streams x %d frames (spb %d), T = %d, float32 rows; %d alternating rounds of %d "
        "calls, median of the rounds' medians (range of the rounds' medians); device %s"
        % (streams, samples, hd.num_samples_per_block, frames, rounds, args.reps, torch.cuda.get_device_name(0)))
    for n in args.windows:
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed + n)
        d_win = torch.stack([torch.randint(0, streams, (n,), device="cuda", generator=g),
                             torch.randint(0, samples - frames + 1, (n,), device="cuda", generator=g)], dim=1)
        out_a = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        out_b = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        st_b = torch.empty((n, 2, 4), dtype=torch.int64, device="cuda")
        st_c = torch.empty((n, 2, 4), dtype=torch.int64, device="cuda")
        keep = {}

        def rows_alone():
            plan.run(corpus, d_win, frames, torch.float32, out=out_a)

        def rows_and_stats():
            plan.run(corpus, d_win, frames, torch.float32, out=out_b, stats=st_b)

        def stats_alone():
            plan.run(corpus, d_win, frames, torch.float32, stats=st_c, rows=False)

        def rows_then_torch():
            y = plan.run(corpus, d_win, frames, torch.float32, out=out_a)
            keep["d"] = (y.square().sum(-1), y.abs().sum(-1), y.abs().amax(-1))

        sides = [rows_alone, rows_and_stats, stats_alone, rows_then_torch]
        for _ in range(3):
            for f in sides:
                f()
        torch.cuda.synchronize()
        times = [[] for _ in sides]
        for _ in range(rounds):
            for t, f in zip(times, sides):
                t.append(call_ms(torch, f, args.reps))
        med = [float(np.median(t)) for t in times]
        rng = [max(t) - min(t) for t in times]
        torch.cuda.synchronize()
        same_rows = bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)))
        same_table = bool(torch.equal(st_b, st_c))
        y16 = plan.run(corpus, d_win, frames, torch.int16).to(torch.int64).abs()
        ref = torch.stack([(y16 * y16).sum(-1), y16.sum(-1), y16.amax(-1), torch.full_like(y16[:, :, 0], frames)], dim=-1)
        exact = bool(torch.equal(st_b, ref))
        del y16, ref
        a, b, c, d = med
        say("  N = %5d: (a) rows %.4f ms (range %.4f); (b) rows + statistics %.4f ms (range %.4f), (b) / (a) = %.3f; (c) statistics "
            "alone %.4f ms (range %.4f), (c) / (a) = %.3f; (d) rows + torch reductions %.4f ms (range %.4f), (d) / (b) = %.2fx; "
            "rows of (b) == (a): %s; table of (b) == (c): %s; table == int64 sums over the int16 rows: %s"
            % (n, a, rng[0], b, rng[1], b / a, c, rng[2], c / a, d, rng[3], d / b, same_rows, same_table, exact))
        results.append(dict(windows=n, a_ms=a, b_ms=b, c_ms=c, d_ms=d, ranges_ms=rng, same_rows=same_rows, same_table=same_table,
                            exact=exact))
        del out_a, out_b, st_b, st_c, keep
        torch.cuda.empty_cache()
    say("")
    say("json " + json.dumps(results))
    plan.close()
    engine.close()


def half_main(args, say):
    import torch
    from aad_amd.capi import LIBRARY_PATH, ApiError
    from aad_amd.engine import Engine, HipEvent, parse_header
    engine = Engine(0)
    samples, frames, streams = int(round(args.seconds * 48000)), args.frames, args.streams
    rounds, results = 5, []
    corpus, size, stride = build_corpus(engine, torch, streams, samples, seed=args.seed)
    hd = parse_header(bytes(corpus[0, :31].cpu().numpy()))
    plan = engine.uniform_window_decode_plan(hd, streams, stride, size)
    dtypes = []
    for dtype in (torch.int16, torch.float32, torch.float16, torch.bfloat16):
        try:
            plan.run(corpus, torch.zeros((1, 2), dtype=torch.int64, device="cuda"), 16, dtype)
            dtypes.append(dtype)
        except ApiError:
            pass  # a library from before the type
    torch.cuda.synchronize()
    say("window decode by sample type: library %s; %d stereo 4-bit streams x %d frames (spb %d), T = %d; kernel times, %d alternating "
        "rounds of %d runs, median of the rounds' medians (range of the rounds' medians); device %s"
        % (os.path.relpath(LIBRARY_PATH, ROOT), streams, samples, hd.num_samples_per_block, frames, rounds, args.reps,
           torch.cuda.get_device_name(0)))
    for n in args.windows:
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed + n)
        d_win = torch.stack([torch.randint(0, streams, (n,), device="cuda", generator=g),
                             torch.randint(0, samples - frames + 1, (n,), device="cuda", generator=g)], dim=1)
        outs = {d: torch.empty((n, 2, frames), dtype=d, device="cuda") for d in dtypes}
        runs = {d: (lambda d=d: plan.run(corpus, d_win, frames, d, out=outs[d])) for d in dtypes}
        for _ in range(3):
            for d in dtypes:
                runs[d]()
        torch.cuda.synchronize()
        times = {d: [] for d in dtypes}
        for _ in range(rounds):
            for d in dtypes:
                times[d].append(kernel_ms(engine, HipEvent, runs[d], args.reps))
        torch.cuda.synchronize()
        say("")
        say("N = %d windows x T = %d" % (n, frames))
        row = {"windows": n, "frames": frames, "library": os.path.relpath(LIBRARY_PATH, ROOT)}
        for d in dtypes:
            med, spread = float(np.median(times[d])), max(times[d]) - min(times[d])
            nbytes = outs[d].numel() * outs[d].element_size()
            exact = None
            if d in (torch.float16, torch.bfloat16):
                exact = bool(torch.equal(outs[d].view(torch.int16), outs[torch.float32].to(d).view(torch.int16)))
            elif d == torch.float32:
                exact = bool(torch.equal(outs[d], outs[torch.int16].float() / 32768))
            name = str(d).replace("torch.", "")
            say("  %-9s kernel %8.4f ms (range %.4f)   %6.1f MB out   %7.1f GB/s (%.3f of 8 TB/s)   rounds %s%s"
                % (name, med, spread, nbytes / 1e6, nbytes / (med * 1e-3) / 1e9, nbytes / (med * 1e-3) / HBM,
                   " ".join("%.4f" % t for t in times[d]), "" if exact is None else "   bit-exact: %s" % exact))
            row[name] = dict(kernel_ms=med, range_ms=spread, rounds_ms=times[d], out_bytes=nbytes, bit_exact=exact)
        results.append(row)
        del outs, runs
        torch.cuda.empty_cache()
    say("")
    say("json " + json.dumps(results))
    plan.close()
    engine.close()


def gain_main(args, say):
    import torch
    from aad_amd.engine import Engine, parse_header
    engine = Engine(0)
    samples, frames, streams = int(round(args.seconds * 48000)), args.frames, args.streams
    rounds, results = 5, []
    corpus, size, stride = build_corpus(engine, torch, streams, samples, seed=args.seed)
    hd = parse_header(bytes(corpus[0, :31].cpu().numpy()))
    plan = engine.uniform_window_decode_plan(hd, streams, stride, size)
    say("window decode with gain: %d stereo 4-bit streams x %d frames (spb %d), T = %d, float32 rows; %d alternating rounds of %d "
        "calls, median of the rounds' medians (range of the rounds' medians); device %s"
        % (streams, samples, hd.num_samples_per_block, frames, rounds, args.reps, torch.cuda.get_device_name(0)))
    for n in args.windows:
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed + n)
        draw = lambda: torch.stack([torch.randint(0, streams, (n,), device="cuda", generator=g),
                                    torch.randint(0, samples - frames + 1, (n,), device="cuda", generator=g)], dim=1)
        win_s, win_n = draw(), draw()
        gs = torch.rand((n,), device="cuda", generator=g) + 0.5
        gn = torch.rand((n,), device="cuda", generator=g) * 0.5 - 0.25
        x = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        y = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        mixed = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        keep = {}

        def plain():
            plan.run(corpus, win_s, frames, torch.float32, out=x)

        def store():
            plan.run(corpus, win_s, frames, torch.float32, out=mixed, gain=gs)

        def add():
            plan.run(corpus, win_n, frames, torch.float32, out=mixed, gain=gn, accumulate=True)

        def store_then_add():
            store()
            add()

        def composite():
            plan.run(corpus, win_s, frames, torch.float32, out=x)
            plan.run(corpus, win_n, frames, torch.float32, out=y)
            keep["d"] = gs[:, None, None] * x + gn[:, None, None] * y

        sides = [plain, store, add, store_then_add, composite]
        for _ in range(3):
            for f in sides:
                f()
        torch.cuda.synchronize()
        times = [[] for _ in sides]
        for _ in range(rounds):
            for t, f in zip(times, sides):
                t.append(call_ms(torch, f, args.reps))
        med = [float(np.median(t)) for t in times]
        rng = [max(t) - min(t) for t in times]
        keep.clear()
        store_then_add()
        plan.run(corpus, win_s, frames, torch.float32, out=x)
        plan.run(corpus, win_n, frames, torch.float32, out=y)
        x.mul_(gs[:, None, None])       # two roundings, in place: the product, then the sum
        y.mul_(gn[:, None, None])
        x.add_(y)
        torch.cuda.synchronize()
        exact = bool(torch.equal(mixed.view(torch.int32), x.view(torch.int32)))
        a, b, c, bc, d = med
        nbytes = n * 2 * frames * 4
        say("  N = %5d (%.1f MB of rows): (a) plain %.4f ms (range %.4f); (b) STORE %.4f ms (range %.4f), (b) / (a) = %.3f; (c) ADD "
            "%.4f ms (range %.4f), (c) / (a) = %.3f; (b)+(c) %.4f ms (range %.4f); (d) two plain runs + torch %.4f ms (range %.4f), "
            "(d) / ((b)+(c)) = %.2fx; rows of (b)+(c) == the two-rounding expression: %s"
            % (n, nbytes / 1e6, a, rng[0], b, rng[1], b / a, c, rng[2], c / a, bc, rng[3], d, rng[4], d / bc, exact))
        results.append(dict(windows=n, a_ms=a, b_ms=b, c_ms=c, bc_ms=bc, d_ms=d, ranges_ms=rng, exact=exact))
        del x, y, mixed, keep
        torch.cuda.empty_cache()
    say("")
    say("json " + json.dumps(results))
    plan.close()
    engine.close()


def placed_main(args, say):
    import torch
    from aad_amd.engine import Engine, parse_header
    engine = Engine(0)
    samples, frames, streams = int(round(args.seconds * 48000)), args.frames, args.streams
    rounds, results = 5, []
    corpus, size, stride = build_corpus(engine, torch, streams, samples, seed=args.seed)
    hd = parse_header(bytes(corpus[0, :31].cpu().numpy()))
    plan = engine.uniform_window_decode_plan(hd, streams, stride, size)
    half, quarter = frames // 2, frames // 4
    say("window decode with spans: %d stereo 4-bit streams x %d frames (spb %d), T = %d, float32 rows; %d alternating rounds of %d "
        "calls, median of the rounds' medians (range of the rounds' medians); device %s"
        % (streams, samples, hd.num_samples_per_block, frames, rounds, args.reps, torch.cuda.get_device_name(0)))
    for n in args.windows:
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed + n)
        win = torch.stack([torch.randint(0, streams, (n,), device="cuda", generator=g),
                           torch.randint(0, samples - frames + 1, (n,), device="cuda", generator=g)], dim=1)
        gain = torch.rand((n,), device="cuda", generator=g) + 0.5
        span = lambda length: torch.stack([torch.full((n,), length, dtype=torch.int64, device="cuda"),
                                           torch.randint(0, frames - length + 1, (n,), device="cuda", generator=g)], dim=1)
        full = torch.stack([torch.full((n,), frames, dtype=torch.int64, device="cuda"), torch.zeros((n,), dtype=torch.int64, device="cuda")], dim=1)
        span_c, span_d = span(half), span(quarter)
        base = torch.rand((n, 2, frames), device="cuda", generator=g) - 0.5
        out_a = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        out_b, out_c = torch.empty_like(out_a), torch.empty_like(out_a)
        out_d, out_e = base.clone(), base.clone()
        tmp = torch.empty((n, 2, quarter), dtype=torch.float32, device="cuda")
        index = (span_d[:, 1, None] + torch.arange(quarter, device="cuda")[None, :])[:, None, :].expand(n, 2, quarter).contiguous()

        def a():
            plan.run(corpus, win, frames, torch.float32, out=out_a, gain=gain)

        def b():
            plan.run(corpus, win, frames, torch.float32, out=out_b, gain=gain, spans=full)

        def c():
            plan.run(corpus, win, frames, torch.float32, out=out_c, gain=gain, spans=span_c)

        def d():
            plan.run(corpus, win, frames, torch.float32, out=out_d, gain=gain, accumulate=True, spans=span_d)

        def e():
            plan.run(corpus, win, quarter, torch.float32, out=tmp)
            out_e.scatter_add_(2, index, gain[:, None, None] * tmp)

        sides = [a, b, c, d, e]
        for _ in range(3):
            for f in sides:
                f()
        torch.cuda.synchronize()
        times = [[] for _ in sides]
        for _ in range(rounds):
            for t, f in zip(times, sides):
                t.append(call_ms(torch, f, args.reps))
        med = [float(np.median(t)) for t in times]
        rng = [max(t) - min(t) for t in times]
        # the rows: (b) == (a); (c) and (d) == the definition over the plain rows, two roundings
        a(), b(), c()
        out_d.copy_(base)
        d()
        x = plan.run(corpus, win, frames, torch.float32)
        x.mul_(gain[:, None, None])
        t_idx = torch.arange(frames, device="cuda")[None, :]
        inside = ((t_idx >= span_c[:, 1, None]) & (t_idx < span_c[:, 1, None] + half))[:, None, :]
        src = (t_idx - span_c[:, 1, None]).clamp(0, frames - 1)[:, None, :].expand(n, 2, frames)
        want_c = torch.where(inside, x.gather(2, src), torch.zeros((), device="cuda"))
        inside = ((t_idx >= span_d[:, 1, None]) & (t_idx < span_d[:, 1, None] + quarter))[:, None, :]
        src = (t_idx - span_d[:, 1, None]).clamp(0, frames - 1)[:, None, :].expand(n, 2, frames)
        shifted = x.gather(2, src)
        shifted.add_(base)              # the second rounding, a kernel of its own
        want_d = torch.where(inside, shifted, base)
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int32)
        exact = [bool(torch.equal(bits(out_b), bits(out_a))), bool(torch.equal(bits(out_c), bits(want_c))),
                 bool(torch.equal(bits(out_d), bits(want_d)))]
        ta, tb, tc, td, te = med
        say("  N = %5d (%.1f MB of rows): (a) RunGain STORE %.4f ms (range %.4f); (b) placed STORE (T, 0) %.4f ms (range %.4f), "
            "(b) / (a) = %.3f; (c) placed STORE L = T/2 %.4f ms (range %.4f), (c) / (a) = %.3f; (d) placed ADD L = T/4 %.4f ms "
            "(range %.4f); (e) plain run of T/4 + torch scatter-add %.4f ms (range %.4f), (e) / (d) = %.2fx; rows: (b) == (a): %s, "
            "(c) == definition: %s, (d) == definition: %s"
            % (n, n * 2 * frames * 4 / 1e6, ta, rng[0], tb, rng[1], tb / ta, tc, rng[2], tc / ta, td, rng[3], te, rng[4], te / td,
               exact[0], exact[1], exact[2]))
        results.append(dict(windows=n, a_ms=ta, b_ms=tb, c_ms=tc, d_ms=td, e_ms=te, ranges_ms=rng, exact=exact))
        del out_a, out_b, out_c, out_d, out_e, tmp, index, base, x, want_c, want_d, inside, src, shifted
        torch.cuda.empty_cache()
    say("")
    say("json " + json.dumps(results))
    plan.close()
    engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--windows", type=int, nargs="+", default=[4096, 64])
    ap.add_argument("--frames", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--mixed", action="store_true", help="the mixed-format plan's two measurements instead (see above)")
    ap.add_argument("--channel-mix", action="store_true", help="the channel-mix plan against what a caller has without it (see above)")
    ap.add_argument("--stats", action="store_true", help="the statistics run against the row run and torch reductions (see above)")
    ap.add_argument("--half", action="store_true", help="the run's kernel per sample type, float16 and bfloat16 included (see above)")
    ap.add_argument("--gain", action="store_true", help="the gain run: STORE, ADD and both against two plain runs + torch (see above)")
    ap.add_argument("--placed", action="store_true", help="the run with spans against the gain run and a plain run + torch (see above)")
    args = ap.parse_args()

    import torch
    from aad_amd.engine import Engine, HipEvent, parse_header
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.mixed or args.channel_mix or args.stats or args.half or args.gain or args.placed:
        (mixed_main if args.mixed else channel_mix_main if args.channel_mix else stats_main if args.stats else
         half_main if args.half else gain_main if args.gain else placed_main)(args, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a" if args.half else "w") as fh:  # --half: one report per library, appended
                fh.write("\n".join(lines) + "\n")
        return

    engine = Engine(0)
    samples = int(round(args.seconds * 48000))
    t0 = time.perf_counter()
    corpus, size, stride = build_corpus(engine, torch, args.streams, samples, seed=args.seed)
    hd = parse_header(bytes(corpus[0, :31].cpu().numpy()))
    spb, bs = hd.num_samples_per_block, hd.block_size
    say("window decode: %d stereo 4-bit streams x %d frames on the device (%.2f GB of images, built in %.1f s); T = %d frames; "
        "spb %d, block %d bytes; median of %d; device %s" % (args.streams, samples, args.streams * stride / 1e9,
                                                             time.perf_counter() - t0, args.frames, spb, bs, args.reps,
                                                             torch.cuda.get_device_name(0)))
    wplan = engine.uniform_window_decode_plan(hd, args.streams, stride, size)
    frames = args.frames
    results = []
    for n in args.windows:
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed + n)
        d_win = torch.stack([torch.randint(0, args.streams, (n,), device="cuda", generator=g),
                             torch.randint(0, samples - frames + 1, (n,), device="cuda", generator=g)], dim=1)
        win = d_win.cpu().numpy()
        table, crop0 = covering_blocks(win, frames, spb, bs, size, samples, stride)
        nblk = len(table)
        out_bytes16, out_bytes32 = n * 2 * frames * 2, n * 2 * frames * 4
        row = {"windows": n, "frames": frames, "covering_blocks": nblk}
        say("")
        say("N = %d windows x T = %d: %d covering blocks (%.2f per window), output %.1f MB int16 / %.1f MB float32"
            % (n, frames, nblk, nblk / n, out_bytes16 / 1e6, out_bytes32 / 1e6))

        # (a) the existing decoder over the covering blocks, plan made beforehand
        pcm_a = {m: torch.zeros(nblk * spb * 2, dtype=torch.int16, device="cuda") for m in ("auto", "dense")}
        dplan = engine.decode_plan(hd, table, False)
        t_a = {}
        for m in ("auto", "dense"):
            engine.set_mapping(m)
            t_a[m] = kernel_ms(engine, HipEvent, lambda: dplan.run(corpus, pcm_a[m]), args.reps)
        engine.set_mapping("auto")
        torch.cuda.synchronize()
        exact_a = bool(torch.equal(pcm_a["auto"], pcm_a["dense"]))
        ref16 = gather(torch, pcm_a["dense"], crop0, frames)
        dplan.close()
        del pcm_a
        torch.cuda.synchronize()

        # (b) today's composite per call
        def composite():
            w = d_win.cpu().numpy()
            t, c0 = covering_blocks(w, frames, spb, bs, size, samples, stride)
            p = engine.decode_plan(hd, t, False)
            pcm = torch.zeros(len(t) * spb * 2, dtype=torch.int16, device="cuda")
            p.run(corpus, pcm)
            res = gather(torch, pcm, c0, frames).float() / 32768
            p.close()
            return res
        t_b = call_ms(torch, composite, args.reps)
        out_b = composite()
        torch.cuda.synchronize()
        exact_b = bool(torch.equal(out_b.view(torch.int32), (ref16.float() / 32768).view(torch.int32)))
        del out_b

        # (c) the window run
        out16 = torch.empty((n, 2, frames), dtype=torch.int16, device="cuda")
        out32 = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda")
        k16 = kernel_ms(engine, HipEvent, lambda: wplan.run(corpus, d_win, frames, torch.int16, out=out16), args.reps)
        k32 = kernel_ms(engine, HipEvent, lambda: wplan.run(corpus, d_win, frames, torch.float32, out=out32), args.reps)
        c16 = call_ms(torch, lambda: wplan.run(corpus, d_win, frames, torch.int16, out=out16), args.reps)
        c32 = call_ms(torch, lambda: wplan.run(corpus, d_win, frames, torch.float32, out=out32), args.reps)
        torch.cuda.synchronize()
        exact_c16 = bool(torch.equal(out16, ref16))
        exact_c32 = bool(torch.equal(out32.view(torch.int32), (ref16.float() / 32768).view(torch.int32)))

        # a few windows against the oracle's decode of the whole stream
        oracle = None
        try:
            import oracle_binding as ob
            oracle = True
            for w in range(min(3, n)):
                s, f = int(win[w, 0]), int(win[w, 1])
                whole = ob.decode(bytes(corpus[s, :size].cpu().numpy()))[0]
                oracle = oracle and np.array_equal(out16[w].cpu().numpy(), whole[f:f + frames].T)
        except (ImportError, OSError):
            pass

        def gbs(nbytes, ms):
            return nbytes / (ms * 1e-3) / 1e9

        say("  (a) bare-block decode, auto   kernel %8.4f ms   int16 interleaved   %7.1f GB/s out (%.3f of 8 TB/s)"
            % (t_a["auto"], gbs(nblk * spb * 4, t_a["auto"]), gbs(nblk * spb * 4, t_a["auto"]) * 1e9 / HBM))
        say("  (a) bare-block decode, dense  kernel %8.4f ms   int16 interleaved   %7.1f GB/s out (%.3f of 8 TB/s)   bit-exact vs auto: %s"
            % (t_a["dense"], gbs(nblk * spb * 4, t_a["dense"]), gbs(nblk * spb * 4, t_a["dense"]) * 1e9 / HBM, exact_a))
        say("  (b) composite per call        call   %8.4f ms   float32 planar      %7.1f GB/s out                    bit-exact: %s"
            % (t_b, gbs(out_bytes32, t_b), exact_b))
        say("  (c) window run, int16         kernel %8.4f ms   call %8.4f ms   %7.1f GB/s out (%.3f of 8 TB/s)   bit-exact: %s"
            % (k16, c16, gbs(out_bytes16, k16), gbs(out_bytes16, k16) * 1e9 / HBM, exact_c16))
        say("  (c) window run, float32       kernel %8.4f ms   call %8.4f ms   %7.1f GB/s out (%.3f of 8 TB/s)   bit-exact: %s"
            % (k32, c32, gbs(out_bytes32, k32), gbs(out_bytes32, k32) * 1e9 / HBM, exact_c32))
        say("  targets: (c) float32 kernel / (a) dense kernel = %.3f (<= 1.25: %s); (c) float32 call / (b) call = %.3f (< 1: %s)"
            "; oracle spot check: %s" % (k32 / t_a["dense"], k32 / t_a["dense"] <= 1.25, c32 / t_b, c32 < t_b, oracle))
        row.update(a_auto_ms=t_a["auto"], a_dense_ms=t_a["dense"], b_call_ms=t_b, c_int16_kernel_ms=k16, c_int16_call_ms=c16,
                   c_float32_kernel_ms=k32, c_float32_call_ms=c32,
                   bit_exact=dict(a=exact_a, b=exact_b, c_int16=exact_c16, c_float32=exact_c32, oracle=oracle))
        results.append(row)
        del out16, out32, ref16
        torch.cuda.synchronize()
    say("")
    say("json " + json.dumps(results))
    wplan.close()
    engine.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
