"""The specification of the device luma (`ops.luma`, the `mf_luma_*` calls): NumPy, integers only.

`luma(frames, red_first=False)` -> uint8 (n, H, W) for four sources:

    (n, H, W, 3) uint8     (b*3735 + g*19235 + r*9798 + 16384) >> 15: OpenCV's 8U COLOR_BGR2GRAY, 15-bit coefficients that sum to 32768;
                           red_first swaps the roles of channels 0 and 2 (COLOR_RGB2GRAY)
    (n, H, W, 4) uint8     the same on channels 0-2; channel 3 is ignored (COLOR_BGRA2GRAY / COLOR_RGBA2GRAY)
    (n, H, W, 3) uint16    y16 = (b*1868 + g*9617 + r*4899 + 8192) >> 14: OpenCV's 16U path, 14-bit coefficients that sum to 16384; the
                           result is y16 >> 8, TRUNCATED
    (n, H, W) uint16       y >> 8: a P010 / P012 / P016 luma plane, whose samples are MSB-aligned

The truncation of a 16-bit value to its high byte is this project's own choice: cv2's FAST takes no 16-bit image, and truncation is the rule
that a P010 plane needs (its low bits are padding or finer steps of the same level).

The constants are RESTATED from memory of OpenCV 4.5-4.10's colour conversion source, not pinned against a cv2 build, like the other cv2
arithmetic in this project: the tests pin the kernel to THIS model, and tests/test_cv2_luma_crosscheck.py compares the model with
cv2.cvtColor wherever a cv2 is installed -- the only place the constants can be settled."""
import numpy as np

B8, G8, R8, SHIFT8 = 3735, 19235, 9798, 15
B16, G16, R16, SHIFT16 = 1868, 9617, 4899, 14
assert B8 + G8 + R8 == 1 << SHIFT8 and B16 + G16 + R16 == 1 << SHIFT16


def luma(frames, red_first=False):
    frames = np.asarray(frames)
    if frames.dtype == np.uint16 and frames.ndim == 3:
        return (frames >> 8).astype(np.uint8)
    if frames.ndim != 4 or (frames.dtype, frames.shape[3]) not in ((np.dtype(np.uint8), 3), (np.dtype(np.uint8), 4), (np.dtype(np.uint16), 3)):
        raise ValueError(f'no luma rule for {frames.dtype} frames of shape {frames.shape}')
    c0, c1, c2 = (frames[..., i].astype(np.int64) for i in range(3))
    b, r = (c2, c0) if red_first else (c0, c2)
    if frames.dtype == np.uint8:
        return ((b * B8 + c1 * G8 + r * R8 + (1 << (SHIFT8 - 1))) >> SHIFT8).astype(np.uint8)
    y16 = (b * B16 + c1 * G16 + r * R16 + (1 << (SHIFT16 - 1))) >> SHIFT16
    return (y16 >> 8).astype(np.uint8)
