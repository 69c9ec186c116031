"""tests/track_model.py's Lucas-Kanade before a judge that owes it nothing (tests/lk_second_opinion.py): scenes whose motion is known in
closed form and a float64 textbook tracker run to its fixed point.  Three layers, each leaning only on the one before it:

  1. the textbook against the truth -- no project code: integer shifts to 1e-6 pixel, and on every table case at least 0.9 of the points
     are `judged` (converged, fixed point within 0.6 pixel of the truth);
  2. the bar from the textbook alone: the same textbook stopped by a cv2-sized rule (30 iterations / 0.01 pixel) stays within BAR = 0.01
     pixel of its own fixed point on every judged point.  That is how far an honest tracker with that stop rule may be from the fixed point,
     and it is cv2's convergence radius and the TOLERANCE of tests/test_cv2_track_crosscheck.py;
  3. the model against the textbook on every judged point: found, within BAR of the fixed point, and no further from the truth than the
     fixed point is plus BAR.

Then eight wrong models, each one edit of track_model's source, must turn at least one of those assertions red: a quarter-pixel bias, a
window offset, swapped weights or a wrong step between levels is shared by model and kernel and invisible to the bit-for-bit tests.
Mutants that only move a last bit are not planted: the textbook cannot see them and the bit-for-bit tests pin them.

Measured here (the table is in profiles/tracker.md): shares 0.90 .. 1.0; cv2-stop at most 0.0082 from the fixed point; the model at most
0.0082 from the fixed point and at most 0.0082 further from the truth than it."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_second_opinion as so  # noqa: E402
import track_model as tm  # noqa: E402


def test_the_table_has_every_pyramid_depth_and_the_issue_s_points():
    assert [len(so.pyramid(np.zeros((h, w), np.uint8))) - 1 for w, h in so.IMAGES] == list(so.DEPTHS) == [0, 1, 2, 3, 1]
    assert len(so.CASES) == 40 and len(set(so.CASES)) == 40
    points, interior = so.grid_points(48, 40)
    assert points[:4].tolist() == [[12.375, 12.625], [23, 12], [34, 12], [12.375, 21.625]] and interior.sum() == 6
    assert points[6:8].tolist() == [[2, 2], [13, 2]] and points[-1].tolist() == [35, 29]
    early, late, truth = so.scene(40, 48, (2.0, -1.0))
    assert early.dtype == late.dtype == np.uint8 and early.shape == (40, 48)
    assert np.array_equal(late[:-1, 2:], early[1:, :-2]) and truth([[3, 4]]).tolist() == [[5, 3]]


@pytest.mark.parametrize('name', so.INTEGER_CASES)
def test_textbook_recovers_integer_shifts_exactly(name):
    ref = so.case_reference(name)
    inner = ref.interior
    assert ref.converged[inner].all()
    error = so.distance(ref.fixed_point, ref.truth)[inner].max()
    print('%s: %d interior points, largest error %.2g' % (name, inner.sum(), error))
    assert error <= 1e-6, error


@pytest.mark.parametrize('name', so.CASES)
def test_textbook_tracks_nine_points_in_ten(name):
    ref = so.case_reference(name)
    print('%s: judged share %.3f of %d points, interior %.3f' % (name, ref.share, len(ref.judged), ref.judged[ref.interior].mean()))
    assert ref.share >= 0.9, ref.share


@pytest.mark.parametrize('name', so.CASES)
def test_a_cv2_sized_stop_rule_stays_within_the_bar_of_the_fixed_point(name):
    ref = so.case_reference(name)
    worst = so.distance(ref.cv2_stop, ref.fixed_point)[ref.judged].max()
    print('%s: max |textbook(stop=cv2) - fixed point| = %.4f over %d judged' % (name, worst, ref.judged.sum()))
    assert worst < so.BAR, worst


@pytest.mark.parametrize('name,rows,cols', so.SUBFRAME_CASES)
def test_the_bar_holds_on_the_subframe_scenes_of_the_device_tests(name, rows, cols):
    for s, ref in enumerate(so.subframe_references(name, rows, cols)):
        worst = so.distance(ref.cv2_stop, ref.fixed_point)[ref.judged].max() if ref.judged.any() else 0.0
        print('%s as %d x %d, sub-frame %d (%d x %d): %d judged of %d, max |textbook(stop=cv2) - fixed point| = %.4f' %
              (name, rows, cols, s, ref.early.shape[1], ref.early.shape[0], ref.judged.sum(), len(ref.judged), worst))
        assert worst < so.BAR, (s, worst)


@pytest.mark.parametrize('name', [n for n in so.CASES if not n.endswith('shift_0_0')])
def test_a_reflected_derivative_border_loses_tracks_the_zero_border_keeps(name):
    """One of the model's three recalled details, settled without cv2: with the derivative image reflected at its border instead of zero
    the same textbook loses tracks the zero border keeps (at the coarse levels by tens to hundreds of pixels)."""
    ref = so.case_reference(name)
    moved, converged = so.textbook_lk(ref.early, ref.late, ref.points, gradient_border='reflect')
    share = so.judged(moved, converged, ref.truth).mean()
    print('%s: judged share %.3f with a zero border, %.3f with a reflected one; worst error %.1f' %
          (name, ref.share, share, so.distance(moved, ref.truth).max()))
    assert share < ref.share


def judge(lk_track, name):
    ref = so.case_reference(name)
    moved, found = lk_track(ref.early, ref.late, ref.points.astype(np.float32))
    return so.assert_verdict(ref, moved, found, name)


@pytest.mark.parametrize('name', so.CASES)
def test_model_against_textbook_and_truth(name):
    judge(tm.lk_track, name)


@pytest.mark.parametrize('name,rows,cols', so.SUBFRAME_CASES)
def test_model_against_textbook_and_truth_in_subframes(name, rows, cols):
    for s, ref in enumerate(so.subframe_references(name, rows, cols)):
        moved, found = tm.lk_track(ref.early, ref.late, ref.points.astype(np.float32))
        so.assert_verdict(ref, moved, found, '%s as %d x %d, sub-frame %d' % (name, rows, cols, s))


def rewritten_model(old, new, times=1):
    """track_model with one piece of its source replaced; the piece must occur exactly `times`, so that an edit of the model cannot turn
    a mutant into the model itself unnoticed."""
    with open(tm.__file__) as f:
        source = f.read()
    assert source.count(old) == times, (old, source.count(old))
    module = types.ModuleType('track_model_rewritten')
    exec(compile(source.replace(old, new), tm.__file__, 'exec'), module.__dict__)
    return module


MUTANTS = {
    'derivative border reflected instead of zero':
        ('np.pad(dx.astype(np.int64), _PAD)\n        pad_dy = np.pad(dy.astype(np.int64), _PAD)',
         'dx.astype(np.int64)[ry][:, rx]\n        pad_dy = dy.astype(np.int64)[ry][:, rx]'),
    'HALF 10.5 instead of 10': ('HALF = F32(10.0)', 'HALF = F32(10.5)'),
    'w01 and w10 swapped': ('return w00, w01, w10, (1 << W_BITS)', 'return w00, w10, w01, (1 << W_BITS)'),
    'moved * 2 between levels left out': ('else moved * F32(2.0)', 'else moved * F32(1.0)'),
    'the sign of delta flipped': ('delta = np.stack([', 'delta = -np.stack(['),
    'the derivatives taken from the late level': ('dx, dy = scharr(img)', 'dx, dy = scharr(nxt_img)'),
    'the patch descaled by one bit too few': ('patch = _bilinear(pad_i, ip[:, 0], ip[:, 1], w4, W_BITS - 5)',
                                              'patch = _bilinear(pad_i, ip[:, 0], ip[:, 1], w4, W_BITS - 6)'),
    'the late patch read one pixel to the right': ('_bilinear(pad_j, ipos[:, 0], ipos[:, 1], w4, W_BITS - 5)',
                                                   '_bilinear(pad_j, ipos[:, 0] + 1, ipos[:, 1], w4, W_BITS - 5)'),
}


def test_the_rewriting_itself_changes_nothing():
    same = rewritten_model('HALF = F32(10.0)', 'HALF = F32(10.0)')
    ref = so.case_reference('96x88-affine')
    for got, want in zip(same.lk_track(ref.early, ref.late, ref.points.astype(np.float32)),
                         tm.lk_track(ref.early, ref.late, ref.points.astype(np.float32))):
        assert np.array_equal(got, want)


@pytest.mark.parametrize('what', list(MUTANTS))
def test_wrong_models_are_rejected(what):
    """(How many of the 40 cases each mutant turns red: profiles/tracker.md.  Here the first red case ends the search.)"""
    wrong = rewritten_model(*MUTANTS[what])
    for name in so.CASES:
        try:
            with np.errstate(all='ignore'):
                judge(wrong.lk_track, name)
        except AssertionError as e:
            print('%s: red on %s' % (what, e.args[0]))
            return
    pytest.fail('no assertion turned red for: ' + what)
