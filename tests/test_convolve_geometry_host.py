"""tests/convolve_rows_oracle.py, with no GPU: the closed form against tests/convolve_oracle.py's definition, the wrappers against
the originals, the conditions on the case tables of tests/test_gpu_convolve_geometry.py, and - on small stand-ins of the same
structure, in numpy alone - that each wrong kernel the GPU file is meant to catch gives other bits among the elements it compares:
  (a) the previous item's response or shift used for the next item          test_item_loop
  (b) the read bound taken as T_src where the pitch is larger               test_shift_past_the_lead, test_source_placement
  (c) an odd row read from one element early                                test_source_placement, test_past_4_gib
  (d) a row offset taken mod 2^32 elements (here: mod 2^20)                 test_past_4_gib
  (e) n sign-wrapped at 2^31 (here: at 2^11)                                test_index_limit"""
import itertools

import numpy as np

import convolve_matrix as cm
import convolve_oracle as co
import convolve_rows_oracle as cr
import window_placed_oracle as po

BOTH = ("int16", "float32")


def _bits(acc, qs, name):
    return np.stack([co.element_bits(acc[r], int(qs[r]), name) for r in range(len(acc))])


def _differ(a, b, qs, names=BOTH):
    """per row: the elements of acc a differ from those of acc b in every type of `names`"""
    return np.logical_and.reduce([(_bits(a, qs, name) != _bits(b, qs, name)).any(axis=1) for name in names])


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def test_the_recurrence_is_the_definition():
    assert co.quantise(cr.RECURRENCE_RESPONSE) is not None
    taps, q, delay = co.quantise(cr.RECURRENCE_RESPONSE)
    assert (tuple(taps.tolist()), q, delay) == (cr.RECURRENCE_TAPS, cr.RECURRENCE_Q, cr.RECURRENCE_DELAY)
    taps1, q1, d1 = co.quantise([1.0])
    assert (tuple(taps1.tolist()), q1, d1) == (cr.UNIT_TAPS, cr.UNIT_Q, 0)
    rng = np.random.default_rng(13)
    frames = 300
    for size in (frames + 2, frames + 7, 40):
        x = cr.source_rows(rng, 1, size)[0]
        x[:6] = [32767, -32768, 32767, -32768, -32768, 32767]  # 3 * 32767 + 2 * 32768 + 32767 and its mirror: both clamps
        for shift in (0, 1, 2, 5):
            acc = co.sums(x, shift, frames, taps, delay)
            v = cr.recurrence(x, shift, frames)
            assert v.dtype == np.int64 and np.array_equal(acc, 8192 * v), (size, shift)
            assert np.array_equal(cr.recurrence_int16(v).astype(np.int16).view(np.uint16), co.element_bits(acc, q, "int16"))
            f = (v.astype(np.float32) * np.float32(2.0 ** -15)).view(np.uint32)
            assert np.array_equal(f, co.element_bits(acc, q, "float32"))
            for lo, hi in ((0, 1), (1, 17), (17, frames), (frames, frames), (frames - 1, frames)):  # chunks are slices of the whole
                assert np.array_equal(cr.recurrence(x, shift, frames, lo, hi), v[lo:hi]), (size, shift, lo, hi)
            assert (np.abs(v) > 32767).any() and (v != 0).any()
            # the unit response: the row is the source slice
            unit = co.sums(x, shift, frames, taps1, 0)
            want = np.zeros(frames, dtype=np.int16)
            want[:max(min(size - shift, frames), 0)] = x[shift:shift + frames]
            assert np.array_equal(co.element_bits(unit, q1, "int16"), want.view(np.uint16))


def test_the_recurrence_runs_on_torch_tensors():
    import torch
    x = cr.source_rows(np.random.default_rng(5), 1, 1000)[0]
    want = cr.recurrence(x, 2, 990, 100, 990)
    got = cr.recurrence(torch.from_numpy(x), 2, 990, 100, 990, xp=torch, device="cpu")
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    assert np.array_equal(cr.recurrence_int16(got, torch).numpy(), cr.recurrence_int16(want))


def test_expected_acc_is_sums_over_the_whole_pitch():
    hs, delays = cr.place_responses()
    responses = cr.quantised(hs[:3], delays[:3])
    frames, channels = 50, 2
    t_src = co.source_frames(frames, responses)
    rng = np.random.default_rng(7)
    lanes = np.array([(0, 0), (1, 63), (2, 32), (1, 70), (cr.NO_RESPONSE, 3), (3, 0), (2, 1 << 31), (1, (1 << 32) - 1), (2, t_src + 5)],
                     dtype=np.int64)
    src = cr.pitched(cr.source_rows(rng, len(lanes) * channels, t_src), t_src, 9)
    acc = cr.expected_acc(src, lanes, responses, frames, channels)
    for w, (r, shift) in enumerate(lanes.tolist()):
        for c in range(channels):
            want = co.sums(src[w * channels + c], shift, frames, responses[r][0], responses[r][2]) if r < 3 else np.zeros(frames, dtype=np.int64)
            assert np.array_equal(acc[w, c], want), (w, c)
    assert not acc[4].any() and not acc[5].any() and not acc[6].any() and not acc[7].any()
    assert acc[3].any() and acc[8].any()  # past the lead: the surplus is source
    assert cr.lane_scales(lanes, responses).tolist() == [responses[r][1] if r < 3 else 0 for r in lanes[:, 0].tolist()]
    assert cr.device_lanes(lanes).dtype == np.int32 and cr.device_lanes(lanes)[7].tolist() == [1, -1]
    assert cr.device_lanes(lanes)[4, 0] == -1 and cr.device_lanes(lanes)[6].tolist() == [2, -(1 << 31)]


def test_run_expected_equals_the_originals():
    import torch
    rng = np.random.default_rng(23)
    rows, frames = 14, 40
    acc = rng.integers(-(1 << 40), 1 << 40, size=(rows, frames))
    acc[3] = 0
    qs = np.arange(rows) % 16
    spans = cr.spans_for(rows, frames)
    assert (0, 0) in [tuple(s) for s in cr.spans_for(12, 9).tolist()] and (4, 5) in [tuple(s) for s in cr.spans_for(12, 9).tolist()]
    gains = rng.uniform(-2, 2, size=rows).astype(np.float32)
    gains[:4] = [1.0, -1.0, 0.0, -0.5]
    le, o = cr.clipped_rows(spans, rows, frames, 1)
    pairs = po.clipped(spans, rows, frames)
    assert [p[0] for p in pairs] == le.tolist() and [p[1] for p in pairs] == o.tolist()
    e = torch.arange(rows * frames, dtype=torch.int64).reshape(rows, frames) + (1 << 33)
    rows32 = np.stack([co.to_float32(acc[r], int(qs[r])) for r in range(rows)])[:, None, :]
    for run in cr.RUNS:
        kind, name, add = run
        old = cr.old_pattern(e, name) if add else None
        got = cr.bit_view(cr.run_expected(run, acc, qs, le, o, gains, old)).numpy()
        if kind == "rows":
            want = _bits(acc, qs, name)
        else:
            old_bits = None if old is None else cr.bit_view(old).numpy().view(np.uint32 if name == "float32" else np.uint16)[:, None, :]
            want = po.placed_expected(rows32, spans, gains, name, old_bits)[:, 0]
        assert np.array_equal(got.view(want.dtype), want), run


def test_runs_are_the_ten_fir_kernels():
    assert len(cr.RUNS) == 10 and len({cr.run_id(r) for r in cr.RUNS}) == 10
    fir = {(c.kernel, c.args) for c in cm.cells() if c.kernel != "convolve_resolve_kernel"}
    assert len(fir) == len(cm.cells()) - 1 == 10
    assert {cr.kernel_of(run) for run in cr.RUNS} == fir


def test_geometry_constants():
    assert cr.TILE == 16 * cr.BLOCK and [cr.steps(K) for K in (1, 49, 50, 1000, 4081, 4082)] == [1, 1, 2, 16, 64, 65]
    assert [cr.pieces(K) for K in (1, 4081, 4082, 32768)] == [1, 1, 2, 9]


# ---- a, b. placement and the surplus ---------------------------------------------------------------------------------------------------
def _place(frames):
    hs, delays = cr.place_responses()
    responses = cr.quantised(hs, delays)
    assert [len(r[0]) for r in responses] == list(cr.PLACE_TAPS) and [r[2] for r in responses] == list(cr.PLACE_DELAYS)
    return responses, co.source_frames(frames, responses)


def test_placement_tables():
    for frames in cr.PLACE_FRAMES:
        responses, t_src = _place(frames)
        assert t_src % 2 == 0 and [(t_src + e) % 2 for e in cr.PLACE_EXTRAS] == [0, 1, 1]  # both surplus pitches are odd
        assert len({r[1] for r in responses}) >= 4 and [cr.steps(len(r[0])) for r in responses] == [1, 2, 2, 16, 66]
        lead = cr.leads(responses)
        assert lead == [0, 63, 32, 666, 2799]
        lanes = cr.place_lanes(responses)
        for r, shift in lanes[:-1].tolist():
            assert 0 <= shift <= lead[r] and shift + frames - 1 + responses[r][2] < t_src  # the last frame read lies below T_src
        assert lanes[-1, 0] == cr.NO_RESPONSE and {(r, lead[r]) for r in range(5)} <= {tuple(v) for v in lanes.tolist()}
    assert cr.SURPLUS == max(cr.PLACE_EXTRAS)


def test_a_bound_at_t_src_or_an_early_odd_row_changes_the_compared_rows():
    """mutants (b) and (c)"""
    frames = cr.PLACE_FRAMES[0]
    responses, t_src = _place(frames)
    pitch = t_src + cr.SURPLUS
    lanes = cr.past_lead_lanes(responses, pitch)
    qs = cr.lane_scales(lanes, responses)
    rng = np.random.default_rng(257)
    src = cr.pitched(cr.source_rows(rng, len(lanes), t_src), t_src, cr.SURPLUS)
    right = cr.expected_acc(src, lanes, responses, frames, 1)[:, 0]
    cut = src.copy()
    cut[:, t_src:] = 0  # (b): nothing is read from t_src on
    wrong = cr.expected_acc(cut, lanes, responses, frames, 1)[:, 0]
    lead = cr.leads(responses)
    differs = _differ(right, wrong, qs)
    for w, (r, shift) in enumerate(lanes.tolist()):
        reads = shift < pitch + lead[r] and shift + frames - 1 + responses[r][2] >= t_src  # some output reads a surplus frame
        assert reads or not differs[w]
        if r == 4 and shift in (lead[r] + cr.SURPLUS - 1, lead[r] + cr.SURPLUS):
            assert differs[w], (r, shift)
        if r == 4 and shift == lead[r] + 1:  # the last output alone reads the one surplus frame, under tap 0
            assert np.array_equal(right[w, :-1], wrong[w, :-1]) and right[w, -1] - wrong[w, -1] == responses[r][0][0] * src[w, t_src]
            assert _differ(right[w:w + 1], wrong[w:w + 1], qs[w:w + 1], ("float32",))[0]
        if shift == pitch and lead[r] > 0:
            assert differs[w] and not right[w, lead[r]:].any(), (r, shift)
        if shift >= (1 << 31) - 1:
            assert not right[w].any()  # a 32-bit j would wrap back into the row
            wrapped = co.sums(src[w], (shift + (1 << 31)) % (1 << 32) - (1 << 31), frames, responses[r][0], responses[r][2])
            if shift == (1 << 32) - 1:
                assert wrapped.any()  # shift -1: the row again
    # (c): the placements of test_source_placement - a row at an odd element offset read from one element early
    lanes = cr.place_lanes(responses)[:-1]
    qs = cr.lane_scales(lanes, responses)
    base = cr.source_rows(rng, len(lanes), t_src)
    for parity, extra in itertools.product((0, 1), cr.PLACE_EXTRAS):
        p = t_src + extra
        flat = np.concatenate([np.zeros(parity + 1, dtype=np.int16), cr.pitched(base, t_src, extra).reshape(-1)])
        rows = np.stack([flat[1 + parity + r * p:][:p] for r in range(len(lanes))])
        early = np.stack([flat[1 + parity + r * p - ((parity + r * p) & 1):][:p] for r in range(len(lanes))])
        right = cr.expected_acc(rows, lanes, responses, frames, 1)[:, 0]
        assert np.array_equal(right, cr.expected_acc(base, lanes, responses, frames, 1)[:, 0])  # the placement changes nothing
        odd = np.array([(parity + r * p) & 1 for r in range(len(lanes))]) == 1
        assert odd.all() if extra == 0 and parity else not odd.any() if extra == 0 else (odd.any() and not odd.all())
        assert _differ(right, cr.expected_acc(early, lanes, responses, frames, 1)[:, 0], qs)[odd].all(), (parity, extra)


# ---- c. the item loop ------------------------------------------------------------------------------------------------------------------
def test_item_table():
    hs, delays = cr.item_responses()
    responses = cr.quantised(hs, delays)
    assert [len(r[0]) for r in responses[1:]] == list(cr.ITEM_KINDS[1:]) and responses[0][0].tolist() == list(cr.UNIT_TAPS)
    assert [cr.steps(K) for K in cr.ITEM_KINDS[1:]] == [1, 1, 16, 65] and [cr.pieces(K) for K in cr.ITEM_KINDS[1:]] == [1, 1, 1, 2]
    # the staged words of a tile of 9 outputs differ between the kinds with a response
    assert len({(cr.BLOCK + cr.STEP_TAPS * min(cr.steps(K), cr.PIECE_STEPS)) // 4 for K in cr.ITEM_KINDS[2:]}) == 3
    pairs = cr.item_pairs()
    assert pairs.shape == (cr.ITEM_EXTRA, 2) and cr.ITEM_EXTRA == 1024
    count = {p: 0 for p in itertools.product(range(5), repeat=2)}
    for p in pairs.tolist():
        count[tuple(p)] += 1
    assert len(count) == 25 and min(count.values()) >= 32
    assert cr.item_rows() == cr.GRID + 1024 and cr.ITEM_FRAMES <= cr.TILE  # one item a row: item b + 2^20 is workgroup b's second
    lanes, designed = cr.item_lanes(responses)
    assert lanes.shape == (cr.item_rows(), 2) and len(designed) == 2048
    lead = cr.leads(responses)
    for b in range(cr.ITEM_EXTRA):
        for j in range(2):
            k, (r, shift) = int(pairs[b, j]), lanes[j * cr.GRID + b].tolist()
            assert designed[j * cr.ITEM_EXTRA + b] == j * cr.GRID + b
            assert (r == cr.NO_RESPONSE) if k == 0 else (r == k and 0 <= shift <= lead[k] + 2)
    rest = np.ones(cr.item_rows(), dtype=bool)
    rest[designed] = False
    assert (lanes[rest, 0] == 0).all() and np.array_equal(lanes[rest, 1], np.arange(cr.item_rows())[rest] % 4)
    spans = cr.spans_for(cr.item_rows(), cr.ITEM_FRAMES)[designed]
    assert (spans == (0, 0)).all(axis=1).sum() >= 64 and (spans == (4, 5)).all(axis=1).sum() >= 64


def test_a_kept_response_or_shift_changes_the_second_item():
    """mutant (a), on the first 100 workgroups of the table: four of every ordered pair"""
    hs, delays = cr.item_responses()
    responses = cr.quantised(hs, delays)
    lanes, _ = cr.item_lanes(responses)
    T = cr.ITEM_FRAMES
    t_src = co.source_frames(T, responses)
    assert t_src == T + 4081
    B = 100
    first, second = lanes[:B], lanes[cr.GRID:cr.GRID + B]
    src = cr.source_rows(np.random.default_rng(100), B, t_src)  # the second items' source rows
    qs = cr.lane_scales(second, responses)
    right = cr.expected_acc(src, second, responses, T, 1)[:, 0]
    kept = first[:, 0] != cr.NO_RESPONSE
    stale = np.where(kept[:, None], first, second)  # the first item's response and shift over the second item's row
    wrong = cr.expected_acc(src, stale, responses, T, 1)[:, 0]
    changed = kept & ((first != second).any(axis=1))
    assert changed.sum() >= 70 and _differ(right, wrong, qs)[changed].all()
    only_shift = changed & (first[:, 0] == second[:, 0])
    assert only_shift.sum() >= 8
    # and a second item without a response after one with: zeros, which the first item's rows are not
    none_after = kept & (second[:, 0] == cr.NO_RESPONSE)
    assert none_after.sum() >= 16 and not right[none_after].any() and wrong[none_after].any(axis=1).all()


# ---- d. the 2^31 limit -----------------------------------------------------------------------------------------------------------------
def test_limit_shape():
    T = cr.LIMIT_FRAMES
    K = len(cr.RECURRENCE_TAPS)
    assert T > 1 << 31 and T + K - 1 <= (1 << 32) - 1
    assert T % cr.TILE == 77 and 77 <= cr.BLOCK and 2 * ((T - 1) // cr.TILE + 1) > cr.GRID  # 2 rows: the item loop runs too
    assert max(cr.LIMIT_SHIFTS) == K - 1 and all(T - o > 1 << 31 for o in cr.LIMIT_OFFSETS)
    assert [o % cr.TILE for o in cr.LIMIT_OFFSETS] == [1, 1] and cr.LIMIT_OFFSETS[1] > cr.TILE


def test_a_sign_wrapped_index_changes_the_row():
    """mutant (e), wrapped at 2^11 instead of 2^31: T = 2^11 + 256 + 77"""
    half = 1 << 11
    T = half + 256 + 77
    x = cr.source_rows(np.random.default_rng(31), 1, T + 2)[0]
    for shift in cr.LIMIT_SHIFTS:
        v = cr.recurrence(x, shift, T)
        n = np.arange(T)
        wrapped = np.where(n >= half, n - 2 * half, n)  # n as a signed 12-bit value
        j = shift + wrapped
        xz = np.concatenate([x.astype(np.int64), np.zeros(3, dtype=np.int64)])  # index -1, -2: the zeros behind the row
        at = lambda i: np.where((i >= 0) & (i < len(x)), xz[np.clip(i, -3, len(x) - 1)], 0)
        wrong = 3 * at(j) - 2 * at(j - 1) + at(j - 2)
        assert np.array_equal(wrong[:half], v[:half]) and not wrong[half:].any()
        for name in BOTH:
            bits = lambda u: co.element_bits(8192 * u, cr.RECURRENCE_Q, name)
            assert (bits(wrong)[half:] != bits(v)[half:]).sum() > (T - half) * 0.99, (shift, name)
            assert (bits(wrong)[T - 77:] != bits(v)[T - 77:]).any()  # the last tile


# ---- e. past 4 GiB ---------------------------------------------------------------------------------------------------------------------
def test_big_placements():
    T, rows, pitch = cr.BIG_FRAMES, 2 * cr.BIG_WINDOWS, cr.big_pitch()
    hs, delays = cr.big_responses()
    responses = cr.quantised(hs, delays)
    assert [len(r[0]) for r in responses] == list(cr.BIG_TAPS) and responses[0][0].tolist() == list(cr.UNIT_TAPS)
    t_src = co.source_frames(T, responses)
    assert T == cr.TILE + 3 and t_src == T + 64 and pitch > t_src and pitch % 2 == 1 and 3 + T <= pitch
    tiles = (T - 1) // cr.TILE + 1
    assert rows * T > 1 << 32 and rows * pitch > 1 << 32 and rows * tiles > 1 << 21 and tiles == 2
    assert rows - -(-(1 << 32) // T) >= 64  # rows wholly above element 2^32 of the output
    witnesses = cr.big_witness_windows()
    assert len(witnesses) == len(set(witnesses.tolist())) == cr.BIG_WITNESSES and witnesses.max() == rows // 2 - 1 and witnesses.min() == 0
    w = set(witnesses.tolist())
    for name, (p, elements) in cr.big_boundaries().items():
        for e in elements:
            r = e // p
            assert e % p != 0 and (r + 1) * p <= rows * p and {q // 2 for q in range(r - 16, r + 17)} <= w, (name, e)  # row r straddles it
    below = sum(1 for v in w if (2 * v + 2) * pitch <= 1 << 32 and (2 * v + 2) * T <= 1 << 32)
    past_out = sum(1 for v in w if 2 * v * T >= 1 << 32)
    past_source = sum(1 for v in w if 2 * v * pitch >= 1 << 32)
    assert below >= 64 and past_out >= 16 and past_source >= 24


def test_a_row_offset_narrowed_to_32_bits_reads_another_row():
    """mutant (d), narrowed to 20 bits instead of 32: 300 rows of the 4 GiB case's pitch"""
    hs, delays = cr.big_responses()
    responses = cr.quantised(hs, delays)
    T, pitch, rows, M = cr.BIG_FRAMES, cr.big_pitch(), 300, 1 << 20
    assert rows * pitch > M and rows * T > M
    rng = np.random.default_rng(20)
    flat = cr.source_rows(rng, 1, rows * pitch + 1)[0][1:]  # the source pointer at parity 1
    src = flat.reshape(rows, pitch)
    assert (src[1:, :32] != src[:-1, :32]).any(axis=1).all()  # neighbouring rows have different data
    lanes = np.array([(r % 4, r % 3) for r in range(rows)], dtype=np.int64)
    qs = cr.lane_scales(lanes, responses)
    narrowed = np.stack([flat[(r * pitch) % M:][:pitch] for r in range(rows)])
    right = cr.expected_acc(src, lanes, responses, T, 1)[:, 0]
    wrong = cr.expected_acc(narrowed, lanes, responses, T, 1)[:, 0]
    past = np.arange(rows) * pitch >= M
    assert past.sum() >= 40 and (~past).sum() >= 200
    assert np.array_equal(right[~past], wrong[~past]) and _differ(right, wrong, qs)[past].all()
    # the bulk rows - the unit response - are their own source slice, so a bulk row of another row's data differs as well
    unit = lanes[:, 0] == 0
    assert (unit & past).sum() >= 10
    for r in np.nonzero(unit)[0].tolist():
        s = int(lanes[r, 1])
        assert np.array_equal(co.element_bits(right[r], cr.UNIT_Q, "int16"), src[r, s:s + T].view(np.uint16))
