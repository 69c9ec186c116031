"""The two pieces of `OnlineSession` that need no GPU: `online.hold_frames`, the bookkeeping of the pixels a lagged session still owes, on every
small count of held, new and final frames; and the one list of what a shot carries (`online._CARRIED`), through `reset()`, `_snapshot()` and
`_restore()` of a session on a stub stabilizer."""
import itertools

import pytest

torch = pytest.importorskip('torch')

TRAILING = {'a stack': [(2, 3)], 'a pair': [(2, 3), (1, 2, 2)]}


def stacks(trailing, first, count):
    """One plane stack per trailing shape, `count` frames each; every element of frame i of plane j is 16 * j + first + i + 1."""
    return tuple(torch.stack([torch.full(shape, 16 * j + first + i + 1, dtype=torch.uint8) for i in range(count)]) if count
                 else torch.empty((0,) + shape, dtype=torch.uint8) for j, shape in enumerate(trailing))


def storage(t):
    """[begin, end) of the tensor's bytes in memory."""
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


@pytest.mark.parametrize('form', sorted(TRAILING))
def test_hold_frames_on_every_small_count(form):
    from meshflow_amd import online
    trailing, cases = TRAILING[form], 0
    for h, n in itertools.product(range(4), range(1, 5)):
        for m in range(h + n + 1):
            held, new = (stacks(trailing, 0, h) if h else None), stacks(trailing, h, n)
            held_before = [x.clone() for x in held] if h else []
            final, kept = online.hold_frames(held, new, m)
            what = (form, h, n, m)
            assert len(final) == len(trailing) and all(int(f.shape[0]) == m for f in final), what
            assert (kept is None) == (m == h + n), what
            for j, want in enumerate(stacks(trailing, 0, h + n)):           # (held, then new): frame i holds i + 1
                got = torch.cat([final[j]] + ([kept[j]] if kept is not None else []))
                assert got.dtype == want.dtype and torch.equal(got, want), what
            for k, f in itertools.product(kept or (), new):
                assert storage(k)[1] <= storage(f)[0] or storage(f)[1] <= storage(k)[0], what
            if h == 0 and m >= 1:
                assert [f.data_ptr() for f in final] == [f.data_ptr() for f in new], what
            for x, was in zip(held or (), held_before):
                assert torch.equal(x, was), what
            cases += 1
    assert cases == sum(h + n + 1 for h in range(4) for n in range(1, 5))


class Stub:
    """What `OnlineSession` reads of a stabilizer at construction and in `_start`."""
    mesh_row_count = mesh_col_count = 1
    temporal_smoothing_radius = 2

    def _check_definition(self, definition):
        pass

    def _torch_device(self):
        return torch.device('cpu')

    def device_tracker(self, *args):
        return None


def started():
    from meshflow_amd import online
    session = online.OnlineSession(Stub(), window=3, lag=2, on_cut='reset', on_uncovered='limit')
    session._start(online.ClipForm(None, torch.uint8, (8, 8)), 8, 8)
    return session


NAMES = ('_last_luma', '_last_sig', '_k_prev', '_held', 'emitted')


def carried(session):
    """Every value a shot carries, tensors as (dtype, shape, values), in a form `==` compares."""
    def plain(v):
        if isinstance(v, torch.Tensor):
            return str(v.dtype), tuple(v.shape), v.tolist()
        return tuple(plain(x) for x in v) if isinstance(v, (tuple, list)) else v
    state = session.state
    return {**{name: plain(getattr(session, name)) for name in NAMES}, 'seen': session.seen, 'pending': session.pending,
            'c': plain(state.c), 'q': plain(state.q), 'lam': plain(state.lam), 'state.seen': state.seen}


def test_reset_snapshot_and_restore_cover_everything_a_shot_carries():
    from meshflow_amd import online
    assert set(NAMES) <= set(online._CARRIED)
    session, fresh = started(), carried(started())
    assert fresh == {**dict.fromkeys(NAMES[:4]), 'emitted': 0, 'seen': 0, 'pending': 0, 'state.seen': 0, 'c': ('torch.float64', (2, 8), [[0.0] * 8] * 2),
                     'q': ('torch.float64', (2, 8), [[0.0] * 8] * 2), 'lam': ('torch.float64', (2,), [0.0, 0.0])}
    # whatever else the list may name some day starts from its own entry there
    assert all(getattr(session, name) == start for name, start in online._CARRIED.items())
    session._last_luma = torch.full((8, 8), 7, dtype=torch.uint8)
    session._last_sig = torch.arange(1, 5, dtype=torch.int32)
    session._k_prev = torch.tensor([21], dtype=torch.int32)
    session._held = (torch.full((2, 8, 8), 9, dtype=torch.uint8),)
    session.emitted, session.state.seen, session.shots = 3, 5, 2
    for i, t in enumerate((session.state.c, session.state.q, session.state.lam)):
        t.copy_(torch.arange(1, t.numel() + 1, dtype=torch.float64).reshape(t.shape) + 100 * i)
    filled = carried(session)
    assert all(filled[key] != fresh[key] for key in filled), filled
    saved = session._snapshot()
    session.reset()
    assert carried(session) == fresh
    assert session.shots == 2                                            # (the session's, not the shot's: reset() leaves it)
    session.shots = 4
    session._restore(saved)
    assert carried(session) == filled and session.shots == 2


def test_settings_hold_what_the_first_push_fixes_and_no_state():
    from meshflow_amd import online
    form = online.ClipForm(None, torch.uint8, (8, 8))
    for margin, rectangle in ((0, (0, 0, 7, 7)), (0.2, (1, 1, 6, 6))):
        settings = online.OnlineSettings(Stub(), window=3, crop_margin=margin)
        assert settings.form is None and settings.rectangle is None
        settings.start(form, 8, 8)
        assert settings.form == form and settings.rectangle == rectangle == online.margin_rectangle(margin, 8, 8)
        assert settings.S == 8 and settings.out_size == (8, 8) and (settings.crop is None) == (margin == 0)
        assert not hasattr(settings, 'state') and not set(online._CARRIED) & set(vars(settings)) and not hasattr(settings, 'shots')
    for group in (online.OnlineGroup(Stub(), 3), online.OnlineLagGroup(Stub(), 3, 2, window=3)):
        assert isinstance(group.settings, online.OnlineSettings) and not hasattr(group.settings, 'state')
        assert group.state is None and group.form is None and group.seen == [0] * 3


def test_join_reports_of_an_empty_a_two_frame_and_a_one_frame_part():
    from meshflow_amd import online

    def report(first, values, lost):
        path = torch.tensor(values, dtype=torch.float64).reshape(-1, 1, 1, 1).expand(-1, 2, 2, 2).contiguous()
        return online.OnlineReport(first, path, path + 0.5, (1, 1, 6, 6), torch.tensor([v > 1 for v in values], dtype=torch.bool), lost)

    joined = online.join_reports([report(4, [], [3]), report(0, [1.0, 2.0], []), report(2, [3.0], [2, 5])])
    assert joined.first == 4 and joined.rectangle == (1, 1, 6, 6) and joined.lost == [3, 2, 5]
    assert joined.d_unstab.shape == joined.d_stab.shape == (3, 2, 2, 2) and joined.d_unstab.dtype == joined.d_stab.dtype == torch.float64
    assert joined.d_unstab[:, 0, 0, 0].tolist() == [1.0, 2.0, 3.0] and joined.d_stab[:, 1, 1, 1].tolist() == [1.5, 2.5, 3.5]
    assert joined.covered.dtype == torch.bool and joined.covered.tolist() == [False, True, True]
    # a session's public join is this one, with the frames concatenated beside it
    session = started()
    frames, again = session.join([(torch.full((n, 8, 8), n, dtype=torch.uint8), r) for n, r in
                                  ((0, report(4, [], [3])), (2, report(0, [1.0, 2.0], [])), (1, report(2, [3.0], [2, 5])))])
    assert frames.dtype == torch.uint8 and frames[:, 0, 0].tolist() == [2, 2, 1] and again.first == 4 and again.lost == [3, 2, 5]
    assert torch.equal(again.d_unstab, joined.d_unstab) and torch.equal(again.d_stab, joined.d_stab) and torch.equal(again.covered, joined.covered)


@pytest.mark.parametrize('pair', (False, True), ids=('a stack', 'an NV12 pair'))
def test_the_empty_result(pair):
    from meshflow_amd import online, ops
    settings = online.OnlineSettings(Stub(), window=3, on_uncovered='limit' if pair else 'report')
    settings.start(online.ClipForm(ops._NV12 if pair else None, torch.uint8, (8, 8) if pair else (8, 8, 3)), 8, 8)
    frames, report, k = online.empty_result(settings, 5, [4])
    planes = frames if pair else (frames,)
    assert isinstance(frames, tuple) == pair and all(p.dtype == torch.uint8 for p in planes)
    assert [tuple(p.shape) for p in planes] == ([(0, 8, 8), (0, 4, 4, 2)] if pair else [(0, 8, 8, 3)])
    assert report.first == 5 and report.lost == [4] and report.rectangle == settings.rectangle == (0, 0, 7, 7)
    for path in (report.d_unstab, report.d_stab):
        assert tuple(path.shape) == (0, 2, 2, 2) and path.dtype == torch.float64
    assert report.d_unstab.data_ptr() != report.d_stab.data_ptr() or report.d_unstab is not report.d_stab
    assert tuple(report.covered.shape) == (0,) and report.covered.dtype == torch.bool
    # the limiter's part of it: 0 steps where the session limits, nothing where it does not
    assert (k is None) if not pair else (tuple(k.shape) == (0,) and k.dtype == torch.int32)
