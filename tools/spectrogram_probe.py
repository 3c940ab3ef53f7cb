"""What the spectrogram stage costs and how exact its definition is (DESIGN.md "Spectrogram"), in the style of
tools/convolve_probe.py.

Timing (needs the device).  --windows mono windows (default 1024) of --frames frames (default 64000) drawn from a 4-bit corpus on
the device, through n_fft 512, a 400-sample Hann window, --hop (repeatable; default 160, 441 - one hop off the 16-byte path - and
160 again without filters) and 80 HTK mel filters.  Per line, HIP events on the engine's stream, the median (min - max) of
--steps runs after --warmup:
  stage     AADHip_SpectrogramRun over the decoded int16 batch, with the int8 multiply-accumulates per second it achieves:
            4 N F 64 steps 32 pairs, the matrix's zero padding counted - what the matrix cores are asked for
  decode    AADHip_WindowDecodePlanRun into the int16 batch, and decode + stage together
  composed  the composition the stage replaces, by the same events: decode_windows into float32 rows, torch.stft(center=False),
            abs() ** 2 and a matmul with the filters (the rows padded by n_fft - W so that torch's frames are the stage's), with the peak of torch's allocator above its result
The first window's features are checked against tests/spectrogram_oracle.py.  --out appends the lines to a file.

--mix (needs the device): what the mix costs (DESIGN.md "Spectrogram of a mix"), at the same shape and by the same events: signal
and noise windows drawn from the corpus, a gain per window.  Per hop:
  mix       AADHip_SpectrogramRunMix over the two decoded int16 batches, and the two decodes + the mix together
  stage     AADHip_SpectrogramRun over one of the batches: the floor
  composed  the composition the mix replaces: the signal's rows STORED and gain * noise ADDED into float32 rows by the window
            decode plans, torch.round(32768 x).clamp().to(int16), then AADHip_SpectrogramRun - with the peak of torch's allocator
            above the result
The mix's features are held against the composition's, bit for bit, and window 0's against the oracles.

--accuracy (CPU only): the definition, from the oracle, against a float64 STFT and mel at the same shape on four signals - a
440 Hz tone with noise, quiet noise, a full-scale pure tone and a decoded window of the golden corpus (the synthetic corpus
through the codec's oracle when none is found): the largest and the median |d ln E| over the bands, and for the pure tone the
level below the peak band at which the error first passes 0.1 nat - the coefficient floor."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

N_FFT, WIN, MELS, RATE = 512, 400, 80, 16000


def accuracy(out):
    import spectrogram_oracle as so
    from aad_amd.engine import mel_filters
    window, filters = so.hann(WIN), mel_filters(RATE, N_FFT, MELS)
    rng = np.random.default_rng(1)
    T = 16000
    t = np.arange(T)
    signals = [("440 Hz tone at -12 dB with noise at -40 dB", 8192 * np.sin(2 * np.pi * 440 * t / RATE) + rng.normal(0, 328, T)),
               ("quiet noise at -60 dB", rng.normal(0, 33, T)),
               ("a full-scale 1 kHz tone", 32767 * np.sin(2 * np.pi * 1000 * t / RATE))]
    try:
        import oracle_binding as ob
        from aad_amd.synth import synth_pcm
        pcm = synth_pcm(1, T, 1, seed=3)[0]
        signals.append(("a decoded 4-bit window of the synthetic corpus", ob.decode(ob.encode(pcm, 4, 1024, RATE, False, 0))[0][:T, 0].astype(np.float64)))
    except Exception as e:  # the codec's oracle is not built
        print("no decoded window: %s" % e)
    lines = []
    for name, x in signals:
        x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
        got = so.spectrogram(x, window, N_FFT, 160, filters).astype(np.float64)
        ref = so.reference_float64(x, window, N_FFT, 160, filters)
        ok = (got > 0) & (ref > 0)
        d = np.abs(np.log(got[ok]) - np.log(ref[ok]))
        line = "accuracy  %s: max |d ln E| %.3g, median %.3g over %d of %d elements" % (name, d.max(), np.median(d), ok.sum(), ok.size)
        if "full-scale" in name:
            level = 10 * np.log10(ref / ref.max(axis=1, keepdims=True))
            err = np.where(ok, np.abs(np.log(np.where(ok, got, 1)) - np.log(np.where(ok, ref, 1))), np.inf)
            over = level[err > 0.1]
            line += "; the error passes 0.1 nat from %.1f dB below the peak band down" % (-over.max()) if over.size else "; no band past 0.1 nat"
        lines.append(line)
        print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def mix(args):
    import torch
    import spectrogram_mix_oracle as mo
    import spectrogram_oracle as so
    from aad_amd.capi import make_parameter
    from aad_amd.engine import Engine, mel_filters
    from aad_amd.synth import synth_pcm
    from resample_probe import pcm_decoded, timed_all
    engine = Engine(0, stream=None)
    n, frames = args.windows, args.frames
    samples = frames * 2 + 4096
    pcm = synth_pcm(args.streams, samples, 1, seed=5)
    filters = mel_filters(RATE, N_FFT, MELS)
    lines = []
    fmt = lambda ms: "%.3f ms (%.3f - %.3f)" % (statistics.median(ms), min(ms), max(ms))
    with torch.cuda.stream(engine.stream):
        data, size = engine.encode_uniform(torch.from_numpy(pcm).cuda(), make_parameter(1, 4, 1024, RATE, False, 0))
        plan = engine._corpus_window_plan(data, size, None)
        gen = torch.Generator(device="cuda").manual_seed(11)
        draw = lambda: torch.stack([torch.randint(0, args.streams, (n,), generator=gen, device="cuda"),
                                    torch.randint(0, samples // 2, (n,), generator=gen, device="cuda")], dim=1).contiguous()
        s_windows, n_windows = draw(), draw()
        gains = (torch.rand(n, generator=gen, device="cuda") * 0.9 + 0.05).contiguous()
        ones = torch.ones_like(gains)
        s_rows = torch.empty((n, 1, frames), dtype=torch.int16, device="cuda")
        n_rows = torch.empty((n, 1, frames), dtype=torch.int16, device="cuda")

        def decodes():
            plan.run(data, s_windows, frames, torch.int16, out=s_rows, ordered=False)
            plan.run(data, n_windows, frames, torch.int16, out=n_rows, ordered=False)

        decodes()
        for hop in args.hop or [160, 441]:
            spec = engine.spectrogram(N_FFT, hop, WIN, None, filters)
            F = spec.frames(frames)
            out = torch.empty((n, 1, F, spec.columns), dtype=torch.float32, device="cuda")
            other = torch.empty_like(out)
            run_mix = lambda: spec.run_mix(s_rows, n_rows, other_gain=gains, out=out)
            stage = lambda: spec.run(s_rows, out=other)

            def both():
                decodes()
                run_mix()

            def composed():
                x = plan.run(data, s_windows, frames, torch.float32, gain=ones, ordered=False)
                plan.run(data, n_windows, frames, torch.float32, out=x, gain=gains, accumulate=True, ordered=False)
                return spec.run(torch.round(x * 32768.0).clamp(-32768, 32767).to(torch.int16), out=other)

            t_mix = timed_all(engine.stream, args.steps, args.warmup, run_mix)
            t_stage = timed_all(engine.stream, args.steps, args.warmup, stage)
            t_both = timed_all(engine.stream, args.steps, args.warmup, both)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t_comp = timed_all(engine.stream, args.steps, args.warmup, composed)
            peak = torch.cuda.max_memory_allocated() - before
            run_mix()
            same = bool(torch.equal(composed().view(torch.int32), out.view(torch.int32)))
            crops = []
            for w in (s_windows, n_windows):
                s0, f0 = (int(v) for v in w[0].cpu())
                x = pcm_decoded(engine, data, size, s0)[:, 0]
                crop = np.zeros(frames, dtype=np.int16)
                k = max(0, min(frames, len(x) - f0))
                crop[:k] = x[f0:f0 + k]
                crops.append(crop[None])
            x0 = mo.mix_rows(crops[0], crops[1], 1, None, gains[:1].cpu().numpy())
            want = so.spectrogram(x0[0], so.hann(WIN), N_FFT, hop, filters)
            exact = bool((out[0, 0].cpu().numpy().view(np.uint32) == want.view(np.uint32)).all())
            lines.append("n_fft=%d W=%d H=%d M=%d  N=%d T=%d F=%d  (a) mix %s  two int16 decodes + mix %s  (b) stage over one batch %s  "
                         "(c) float32 STORE + ADD decodes + quantise + stage %s, %.1f MB of temporaries (the mix: the two int16 batches, "
                         "%.1f MB)  mix == composed: %s  exact=%s" % (N_FFT, WIN, hop, MELS, n, frames, F, fmt(t_mix), fmt(t_both), fmt(t_stage),
                                                                    fmt(t_comp), peak / 1e6, 2 * n * frames * 2 / 1e6, same, exact))
            print(lines[-1], flush=True)
            spec.close()
            del out, other
        plan.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=64000)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hop", type=int, action="append")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--mix", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.accuracy:
        return accuracy(args.out)
    if args.mix:
        return mix(args)
    import torch
    import spectrogram_oracle as so
    from aad_amd.capi import make_parameter
    from aad_amd.engine import Engine, mel_filters
    from aad_amd.synth import synth_pcm
    from resample_probe import pcm_decoded, timed_all
    engine = Engine(0, stream=None)
    n, frames = args.windows, args.frames
    samples = frames * 2 + 4096
    pcm = synth_pcm(args.streams, samples, 1, seed=5)
    filters = mel_filters(RATE, N_FFT, MELS)
    lines = []
    fmt = lambda ms: "%.3f ms (%.3f - %.3f)" % (statistics.median(ms), min(ms), max(ms))
    with torch.cuda.stream(engine.stream):
        data, size = engine.encode_uniform(torch.from_numpy(pcm).cuda(), make_parameter(1, 4, 1024, RATE, False, 0))
        plan = engine._corpus_window_plan(data, size, None)
        gen = torch.Generator(device="cuda").manual_seed(11)
        windows = torch.stack([torch.randint(0, args.streams, (n,), generator=gen, device="cuda"),
                               torch.randint(0, samples // 2, (n,), generator=gen, device="cuda")], dim=1).contiguous()
        rows = torch.empty((n, 1, frames), dtype=torch.int16, device="cuda")
        decode = lambda: plan.run(data, windows, frames, torch.int16, out=rows, ordered=False)
        decode()
        d_window = torch.from_numpy(so.hann(WIN)).cuda()
        d_filters = torch.from_numpy(filters).cuda()
        cases = [(h, True) for h in (args.hop or [160, 441])] + [((args.hop or [160])[0], False)]
        for hop, with_filters in cases:
            spec = engine.spectrogram(N_FFT, hop, WIN, None, filters if with_filters else None)
            F = spec.frames(frames)
            out = torch.empty((n, 1, F, spec.columns), dtype=torch.float32, device="cuda")
            stage = lambda: spec.run(rows, out=out)

            def both():
                decode()
                stage()

            def composed():
                x = plan.run(data, windows, frames, torch.float32, ordered=False)
                # torch centres a short window inside n_fft samples: the same frames need the rows padded by n_fft - W
                x = torch.nn.functional.pad(x.view(n, frames), ((N_FFT - WIN) // 2, N_FFT - WIN - (N_FFT - WIN) // 2))
                s = torch.stft(x, N_FFT, hop, WIN, d_window, center=False, return_complex=True)  # [n, B, F]
                p = s.abs() ** 2
                return torch.matmul(d_filters, p).transpose(-1, -2) if with_filters else p.transpose(-1, -2)

            t_stage = timed_all(engine.stream, args.steps, args.warmup, stage)
            t_decode = timed_all(engine.stream, args.steps, args.warmup, decode)
            t_both = timed_all(engine.stream, args.steps, args.warmup, both)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t_comp = timed_all(engine.stream, args.steps, args.warmup, composed)
            peak = torch.cuda.max_memory_allocated() - before - n * F * spec.columns * 4
            s0, f0 = (int(v) for v in windows[0].cpu())
            x = pcm_decoded(engine, data, size, s0)[:, 0]
            crop = np.zeros(frames, dtype=np.int16)
            k = max(0, min(frames, len(x) - f0))
            crop[:k] = x[f0:f0 + k]
            want = so.spectrogram(crop, so.hann(WIN), N_FFT, hop, filters if with_filters else None)
            exact = bool((out[0, 0].cpu().numpy().view(np.uint32) == want.view(np.uint32)).all())
            ref = composed()[0].cpu().numpy()
            ok = (want > 0) & (ref > 0)
            err = float(np.abs(np.log(want[ok].astype(np.float64)) - np.log(ref[ok].astype(np.float64))).max())
            macs = 4.0 * n * F * 64 * ((WIN + 63) // 64) * 32 * ((N_FFT // 2 + 16) // 16)
            ms = statistics.median(t_stage)
            lines.append("n_fft=%d W=%d H=%d M=%d  N=%d T=%d F=%d  stage %s %.1f T int8 MAC/s  decode (int16 batch) %s  decode + stage %s  "
                         "float32 decode + torch.stft + abs()**2%s %s, %.1f MB of temporaries (max |d ln E| of window 0 against the "
                         "stage %.2e)  exact=%s" % (N_FFT, WIN, hop, MELS if with_filters else 0, n, frames, F, fmt(t_stage), macs / ms / 1e9,
                                                    fmt(t_decode), fmt(t_both), " + matmul" if with_filters else "", fmt(t_comp), peak / 1e6, err,
                                                    exact))
            print(lines[-1], flush=True)
            spec.close()
            del out
        plan.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    engine.close()


if __name__ == "__main__":
    main()
