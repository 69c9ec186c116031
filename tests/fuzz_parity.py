"""Randomised parity campaign: HIP kernels vs the C oracle on random geometries (bit-exact or bust).
pixel='u8c3' (the default) draws the original stream; 'u16c3' and 'u8c1' run the same geometries on uint16 BGR frames (against
tests/cv16_model.py) and single-channel frames (against channel 0 of the C oracle on the frame repeated three times), Jacobi cases skipped.
'u8c4' runs them on the BGR frames plus an alpha plane (its samples and its border value from a stream of their own): channels 0-2 against
the oracle on the BGR frames, channel 3 against channel 0 of the oracle on the alpha plane repeated three times.
Usage: python tests/fuzz_parity.py [cases] [seed] [case] [big|-] [u8c3|u16c3|u8c1|u8c4]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from meshflow_amd import ops, synthetic
from oracle import clib, meshflow_oracle as mo



def _pixel_frames(frames, pixel, case):
    """The campaign's uint8 BGR frames as the pixel type under test (from a stream of their own: the campaign's draws stay as they are)."""
    if pixel == 'u8c1':
        return np.ascontiguousarray(frames[..., 0])
    if pixel == 'u16c3':
        return np.random.default_rng(case).integers(0, 65536, frames.shape, dtype=np.uint16)
    if pixel == 'u8c4':
        return np.concatenate([frames, _alpha_stream(case).integers(0, 256, frames.shape[:3] + (1,), dtype=np.uint8)], axis=-1)
    return frames


def _alpha_stream(case):
    """The stream of a u8c4 case's alpha plane and, after it, its alpha border value."""
    return np.random.default_rng([case, 4])


def _rgb(a):
    return np.ascontiguousarray(np.repeat(a[..., None], 3, axis=-1))


def _to_dev(a, dev):
    if a.dtype == np.uint16:
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev).view(torch.uint16)
    return torch.from_numpy(a).to(dev)


def _to_np(t):
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def run(cases=200, seed0=0, only=-1, big=False, pixel='u8c3'):
    """Returns (number of mismatching cases, per-kind counts)."""
    assert pixel in ('u8c3', 'u16c3', 'u8c1', 'u8c4'), pixel
    if pixel == 'u16c3':
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import cv16_model
    dev = torch.device('cuda:0')
    g = np.random.default_rng(seed0)
    bad_cases = 0
    t_start = time.time()
    stats = {'warp': 0, 'warp_degenerate': 0, 'jacobi': 0, 'resize': 0}
    for case in range(cases):
        kind = g.choice(['warp', 'warp', 'warp', 'jacobi', 'resize'])
        if kind == 'warp':
            W = int(g.integers(8, 2100 if big else 420)); H = int(g.integers(8, 1200 if big else 300))
            if g.random() < 0.6:
                W = max(8, W & ~3)                               # the LDS-staged tap path needs W % 4 == 0
            R = int(g.integers(1, min(64 if big else 24, H // 2) + 1)); C = int(g.integers(1, min(64 if big else 24, W // 2) + 1))
            n = int(g.integers(1, 3 if big else 4))
            sigma = float(g.choice([0.2, 1.0, 3.0, 8.0, 25.0])) * min(1.0, min(W / C, H / R) / 20.0 + 0.05)
            frames = synthetic.frames_numpy(n, H, W, seed=case, kind='noise')
            idx = np.arange(n * (R + 1) * (C + 1) * 2, dtype=np.int64).reshape(n, R + 1, C + 1, 2)
            unstab = 2.0 * synthetic.normal(idx, seed=2 * case + 1)
            stab = unstab + sigma * synthetic.normal(idx, seed=2 * case + 2)
            if g.random() < 0.3:                                  # add a global shift so that borders are exercised
                stab = stab + g.normal(0, 6, (n, 1, 1, 2))
            border = tuple(int(v) for v in g.integers(0, 256, 3))
            use_bbox = bool(g.random() < 0.5)
            if only >= 0 and case != only:
                continue
            if pixel == 'u8c1':
                border = (border[0],) * 3
            want, want_crop, bad = clib.warp_clip(frames, R, C, unstab, stab, border_bgr=border, use_bbox=use_bbox or big, openmp=big)
            frames = _pixel_frames(frames, pixel, case)
            if pixel == 'u8c1':
                want = want[..., 0]
            elif pixel == 'u8c4':
                s = _alpha_stream(case)
                s.integers(0, 256, frames.shape[:3], dtype=np.uint8)       # (the alpha plane's draw)
                a = int(s.integers(0, 256))
                border = border + (a,)
                want_a, crop_a, bad_a = clib.warp_clip(_rgb(frames[..., 3]), R, C, unstab, stab, border_bgr=(a, a, a), use_bbox=use_bbox or big,
                                                       openmp=big)
                assert bad_a == bad and (bad or np.array_equal(crop_a, want_crop))
                want = np.concatenate([want, want_a[..., :1]], axis=-1)
            elif pixel == 'u16c3':
                border = tuple(257 * b for b in border)
                if bad == 0:
                    want, want_crop16 = cv16_model.warp_clip_u16(frames, R, C, unstab, stab, border)
                    assert np.array_equal(want_crop16, want_crop)
            table = ops.cell_table(torch.from_numpy(unstab).to(dev), torch.from_numpy(stab).to(dev), W, H, R, C)
            out = ops.warp(_to_dev(frames, dev), table, border)
            torch.cuda.synchronize()
            nbad = int(table.status.item())
            ok = nbad == bad
            if bad == 0:
                ok = ok and np.array_equal(_to_np(out), want) and np.array_equal(table.crop.cpu().numpy(), want_crop)
                stats['warp'] += 1
            else:
                stats['warp_degenerate'] += 1
            desc = f'warp W={W} H={H} R={R} C={C} n={n} sigma={sigma:.2f} degenerate={bad}'
            if only >= 0:
                o = _to_np(out)
                for f in range(n):
                    d = np.argwhere((o[f] != want[f]).reshape(H, W, -1).any(axis=2))
                    print('frame', f, 'differing pixels', len(d), d[:20].tolist())
                    for (yy, xx) in d[:5]:
                        print('   at', yy, xx, 'got', o[f][yy, xx], 'want', want[f][yy, xx])
                print('crop got', table.crop.cpu().numpy().tolist(), 'want', want_crop.tolist())
                tab, _ = clib.cell_table(W, H, R, C, unstab[0], stab[0])
                print('records equal (frame 0):', np.array_equal(table.records().cpu().numpy()[0], tab))
        elif kind == 'jacobi':
            if only >= 0: 
                # keep the random stream in step
                pass
            if pixel != 'u8c3':
                continue
            F = int(g.integers(1, 900)); S = int(g.integers(1, 40)); omega = int(g.choice([1, 2, 5, 10, 10, 30, 30, 17, 40])); iters = int(g.integers(0, 40))
            b = np.cumsum(3.0 * synthetic.normal(np.arange(F * S).reshape(F, S), seed=case), axis=0)
            taps = np.exp(-np.square((3 / omega) * np.arange(-omega, omega + 1)))
            lam = 0.95 * synthetic.uniform01(np.arange(F), seed=case + 7)
            inv_on = 1.0 / (1 + 2 * lam * taps.sum())
            want = clib.jacobi_banded(b, taps, lam, inv_on, omega, iters)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            got = ops.jacobi(t(b), t(taps), t(lam), t(inv_on), omega, iters).cpu().numpy()
            ok = np.array_equal(got, want)
            stats['jacobi'] += 1
            desc = f'jacobi F={F} S={S} omega={omega} iters={iters}'
        else:
            W = int(g.integers(4, 300)); H = int(g.integers(4, 200)); n = int(g.integers(1, 3))
            l = int(g.integers(0, W)); r = int(g.integers(l, W)); tp = int(g.integers(0, H)); bt = int(g.integers(tp, H))
            frames = synthetic.frames_numpy(n, H, W, seed=case, kind='noise')
            if pixel == 'u16c3':
                frames = _pixel_frames(frames, pixel, case)
                want = cv16_model.crop_frames_u16(frames, (l, tp, r, bt))
            else:
                want = np.stack(mo.crop_frames(list(frames), (l, tp, r, bt)))
                if pixel == 'u8c1':
                    want = np.ascontiguousarray(want[..., 0])
                    frames = _pixel_frames(frames, pixel, case)
                elif pixel == 'u8c4':
                    frames = _pixel_frames(frames, pixel, case)
                    want_a = np.stack(mo.crop_frames(list(_rgb(frames[..., 3])), (l, tp, r, bt)))
                    want = np.concatenate([want, want_a[..., :1]], axis=-1)
            got = _to_np(ops.crop_resize(_to_dev(frames, dev), (l, tp, r, bt)))
            ok = np.array_equal(got, want)
            stats['resize'] += 1
            desc = f'resize W={W} H={H} crop=({l},{tp},{r},{bt})'
        if not ok:
            bad_cases += 1
            print('MISMATCH', case, desc, flush=True)
    print(f'{cases} cases in {time.time() - t_start:.1f} s: {stats}, mismatches: {bad_cases}')
    return bad_cases, stats


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    one = int(sys.argv[3]) if len(sys.argv) > 3 else -1            # re-run just this case, verbosely
    big = len(sys.argv) > 4 and sys.argv[4] == 'big'                # frames up to 2100 x 1200, meshes up to 64 x 64
    px = sys.argv[5] if len(sys.argv) > 5 else 'u8c3'
    sys.exit(1 if run(n, sd, one, big, px)[0] else 0)
