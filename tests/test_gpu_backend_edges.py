"""The tracker's back end on the paths tests/test_gpu_ransac.py and tests/test_gpu_hfit.py do not reach, bit for bit against
tests/ransac_model.py and tests/homography_model.py on the cases of tests/backend_edge_cases.py (tests/test_backend_edge_cases.py proves on
the CPU that each reaches its path): `ops.ransac_inliers` at thresholds and confidences other than the defaults and with the iteration rule
saturated at either end, candidate counts of 1,023 .. 1,025 with holes in `found`, non-finite and subnormal `points`, `found` bytes other
than 0 and 1, counts below 0 and at 2^31 - 1; `mf_track_gather_f64` on records that contradict their masks, into buffers the test owns and
surrounds with guards; `ops.fit_homographies` from 1e-150 to 1e100 times pixel scale, on the two flattest clouds on either side of the
collinearity test and on non-finite coordinates; and the three calls chained on the device.  Every call is a legal one."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backend_edge_cases as bc  # noqa: E402
import homography_model as hm  # noqa: E402
import ransac_cases as rc  # noqa: E402
import ransac_model as rm  # noqa: E402
from tracker_clip import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def on_device(dev, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def run_ransac(dev, arrays, **kw):
    from meshflow_amd import ops
    inlier, info = ops.ransac_inliers(*on_device(dev, *arrays), **kw)
    return inlier.cpu().numpy(), info.cpu().numpy()


def same_gather(got, want, what):
    for g, w, name in zip(got, want, ('early', 'late', 'offsets', 'pair_status')):
        same_bits(g.cpu().numpy(), w, (name, what))


# ---- a. threshold and confidence off their defaults -------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def crafted():
    return rc.crafted()


@pytest.mark.parametrize('params', bc.PARAM_SETS)
def test_ransac_off_the_default_threshold_and_confidence(dev, crafted, params):
    threshold, confidence = params
    want_inlier, want_info = rm.ransac_inliers(*crafted, threshold=threshold, confidence=confidence)
    inlier, info = run_ransac(dev, crafted, threshold=threshold, confidence=confidence)
    same_bits(info, want_info, ('info', params))
    same_bits(inlier, want_inlier, ('inlier', params))


@pytest.fixture(scope='module')
def cap_models():
    arrays = bc.cap_launch()
    return arrays, [rm.ransac_inliers(*arrays, threshold=t, confidence=c, max_iters=m) for t, c, m in bc.CAP_RUNS]


@pytest.mark.parametrize('run', range(len(bc.CAP_RUNS)))
def test_ransac_at_the_iteration_cap_and_below_it(dev, cap_models, run):
    """One wavefront, 65,536 iterations where max_iters binds (the rule's n is saturated at 2^17 - 1) and 55,819 where the descent does."""
    import torch
    from meshflow_amd import ops
    arrays, models = cap_models
    threshold, confidence, max_iters = bc.CAP_RUNS[run]
    want_inlier, want_info = models[run]
    assert want_info[0, 0].tolist() == [[rm.OK, 64, 5, 65536], [rm.OK, 64, 5, 55819]][run]
    tensors = on_device(dev, *arrays)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    inlier, info = ops.ransac_inliers(*tensors, threshold=threshold, confidence=confidence, max_iters=max_iters)
    end.record()
    torch.cuda.synchronize()
    print('ransac_inliers, %d iterations of one sub-frame: %.1f ms' % (want_info[0, 0, 3], start.elapsed_time(end)))
    same_bits(info.cpu().numpy(), want_info, 'info')
    same_bits(inlier.cpu().numpy(), want_inlier, 'inlier')


# ---- b. the staging edge ----------------------------------------------------------------------------------------------------------------

def test_ransac_and_gather_on_either_side_of_the_staged_capacity(dev):
    from meshflow_amd import ops
    arrays = bc.staging_launch()
    points, counts, moved, found = arrays
    want_inlier, want_info = rm.ransac_inliers(*arrays)
    assert want_info[:, :, 1].reshape(-1).tolist() == [k for _, k in bc.STAGING] and (want_info[:, :, 0] == rm.OK).all()
    d_points, d_counts, d_moved, d_found = on_device(dev, *arrays)
    inlier, info = ops.ransac_inliers(d_points, d_counts, d_moved, d_found)
    same_bits(info.cpu().numpy(), want_info, 'info')
    same_bits(inlier.cpu().numpy(), want_inlier, 'inlier')
    W, H, rows, cols = bc.STAGING_GRID
    want = rm.gather(points, moved, want_inlier, want_info, ops.track_subframe_grid(W, H, rows, cols), 4)
    same_gather(ops.gather_inliers(d_points, d_moved, inlier, info, W, H, rows, cols, 4), want, 'chained')
    same_gather(ops.gather_inliers(d_points, d_moved, *on_device(dev, want_inlier, want_info), W, H, rows, cols, 4), want, 'fed the model')


# ---- c. hostile sub-frame inputs --------------------------------------------------------------------------------------------------------

def test_ransac_on_hostile_points_found_and_counts(dev):
    arrays = bc.hostile_launch()
    want_inlier, want_info = rm.ransac_inliers(*arrays)
    assert want_info[0, :, 0].tolist() == [rm.OK, rm.OK, rm.TOO_FEW, rm.TOO_FEW, rm.OK, rm.NO_CONSENSUS]
    assert want_info[0, :, 1].tolist() == [72, 57, 0, 0, 72, 72]
    inlier, info = run_ransac(dev, arrays)
    for s, name in enumerate(bc.HOSTILE_NAMES):
        same_bits(info[0, s], want_info[0, s], ('info', name, info[0, s].tolist(), want_info[0, s].tolist()))
        same_bits(inlier[0, s], want_inlier[0, s], ('inlier', name))


# ---- d. records that contradict their masks into the gather -----------------------------------------------------------------------------

def guarded(dev, size):
    """A device buffer of GUARD + size + GUARD bytes, every one the sentinel."""
    import torch
    return torch.full((bc.GUARD + size + bc.GUARD,), bc.SENTINEL, dtype=torch.uint8, device=dev)


@pytest.fixture(scope='module')
def untrusted():
    return bc.untrusted_launch()


@pytest.mark.parametrize('min_features', bc.UNTRUSTED_MIN_FEATURES)
def test_gather_keeps_to_its_runs_whatever_the_records_say(dev, untrusted, min_features):
    """`mf_track_gather_f64` itself, into buffers that held the sentinel: the runs hold what the kernel's header promises, and every other
    byte -- the gaps inside the runs, the entries behind offsets[n], 256 bytes on either side of all four outputs -- is untouched."""
    import torch
    from meshflow_amd import _lib, ops
    points, moved, inlier, info, _ = untrusted
    n, S, size = points.shape[:3]
    W, H, rows, cols = bc.UNTRUSTED_GRID
    want = bc.gather_untrusted(points, moved, inlier, info, ops.track_subframe_grid(W, H, rows, cols), min_features)
    assert want[3].tolist() == {4: [0, 0, 0], 20: [0, rm.PAIR_TOO_FEW, 0]}[min_features]
    d_in = on_device(dev, points, moved, inlier, info)
    entries = n * S * size
    outs = [guarded(dev, 16 * entries), guarded(dev, 16 * entries), guarded(dev, 4 * (n + 1)), guarded(dev, 4 * n)]
    vp = ctypes.c_void_p
    code = _lib.lib.mf_track_gather_f64(*(vp(t.data_ptr()) for t in d_in), n, W, H, rows, cols, size, min_features,
                                        *(vp(t.data_ptr() + bc.GUARD) for t in outs), vp(torch.cuda.current_stream().cuda_stream))
    assert code == _lib.MF_OK, _lib.lib.mf_last_error()
    torch.cuda.synchronize()
    guard = np.full(bc.GUARD, bc.SENTINEL, np.uint8)
    for out, w, name in zip(outs, want, ('early', 'late', 'offsets', 'pair_status')):
        got = out.cpu().numpy()
        same_bits(got[bc.GUARD:-bc.GUARD], np.ascontiguousarray(w).view(np.uint8).reshape(-1), (name, min_features))
        same_bits(got[:bc.GUARD], guard, (name, 'the guard in front', min_features))
        same_bits(got[-bc.GUARD:], guard, (name, 'the guard behind', min_features))


# ---- e. the fit outside pixel scale -----------------------------------------------------------------------------------------------------

def same_bits_but_nans(got, want, what):
    """Bit for bit where the model's value is no NaN; a NaN of any sign and payload where it is one."""
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), (what, got[nan].tolist())
    same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)


def test_fit_from_1e_minus_150_to_1e100_flat_and_non_finite(dev):
    import torch
    from meshflow_amd import ops
    names, early, late, offsets = bc.fit_launch()
    with np.errstate(all='ignore'):
        want = hm.fit_homographies(early, late, offsets)
    assert sorted(set(want[1][:, 0].tolist())) == [hm.OK, hm.COLLINEAR, hm.AT_INFINITY] and len(set(want[1][:, 2].tolist())) >= 2
    got = tuple(t.cpu().numpy() for t in ops.fit_homographies(*on_device(dev, early, late, offsets)))
    fields = ('early scale', 'late scale', 'early cx', 'early cy', 'late cx', 'late cy', 'smallest eigenvalue', 'second eigenvalue')
    for p, name in enumerate(names):
        relaxed = name.split(', K=')[0] in bc.NON_FINITE                 # the one relaxation: diag of the two non-finite pairs
        assert relaxed or not np.isnan(want[2][p]).any(), name
        for i, field in enumerate(fields):
            (same_bits_but_nans if relaxed else same_bits)(got[2][p, i:i + 1], want[2][p, i:i + 1],
                                                           (name, field, float(got[2][p, i]), float(want[2][p, i])))
        same_bits(got[1][p], want[1][p], (name, 'info', got[1][p].tolist(), want[1][p].tolist()))
        same_bits(got[0][p], want[0][p], (name, 'H'))


# ---- f. the chain -----------------------------------------------------------------------------------------------------------------------

def test_ransac_gather_and_fit_chained_on_the_device(dev):
    """The staging launch through all three calls without a visit to the host in between: two pairs of 2,033 and 2,204 survivors."""
    from meshflow_amd import ops
    W, H, rows, cols = bc.STAGING_GRID
    (want_inlier, want_info), want_packed, want_fit = bc.chain_model(ops.track_subframe_grid(W, H, rows, cols))
    assert want_packed[2].tolist() == [0, 2033, 4237] and want_fit[1][:, 0].tolist() == [hm.OK, hm.OK]
    d_points, d_counts, d_moved, d_found = on_device(dev, *bc.staging_launch())
    inlier, info = ops.ransac_inliers(d_points, d_counts, d_moved, d_found, **bc.CHAIN_PARAMS)
    packed = ops.gather_inliers(d_points, d_moved, inlier, info, W, H, rows, cols, 4)
    fit = ops.fit_homographies(*packed[:3])
    same_bits(info.cpu().numpy(), want_info, 'info')
    same_bits(inlier.cpu().numpy(), want_inlier, 'inlier')
    same_gather(packed, want_packed, 'chain')
    for g, w, what in zip(fit, want_fit, ('H', 'fit info', 'diag')):
        same_bits(g.cpu().numpy(), w, what)
