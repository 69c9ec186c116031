"""An independent reference for the warp and the crop-resize, torch only: `grid_sample` and `interpolate` in float64, a coordinate map
computed here in float64, and a judge that returns numbers.  It shares nothing with the project's reading of OpenCV and runs on whatever
device its tensors are on, so the same comparison judges the NumPy / C models on the CPU (tests/test_second_opinion_models.py) and the HIP
kernels on the GPU (tests/test_gpu_torch_crosscheck.py), with the constants below.

The envelope has two separate parts:
  * a COORDINATE HALF-WIDTH in pixels.  Warp: BUCKET = 1/64 (cv2.remap rounds 32 x to an integer) plus a slack for float32 coordinates;
    resize: the slack alone around the exact source position (d + 0.5) src / dst - 0.5.  The slack is counted in float32 ulps of the
    largest source coordinate of the case (`coordinate_ulp`: 2^-14 px up to 1024, 2^-13 px up to 2048), because that is what it is: the
    reference rounds its maps and its vertices (warp) or its source position (resize) to float32, and where that rounding crosses a
    bucket or a source cell the sample moves by the error times the local slope -- up to 65,535 levels per pixel on 16-bit noise.
  * a VALUE ALLOWANCE in LSB of the format: the rounding of the result plus the arithmetic of the format.
The envelope is the exact range of the bilinear sample over that box, not a sampling of it (`envelope`).

How each constant was fixed: on the CPU, against the oracle and the uint16 models (never against a kernel), on the case table below plus
its 1080p cases; the slack ladder was 0, 1/16, 1/8, 1/4, 1/2, 1, 2, 4 ulp, the constant is twice the first rung without a value outside.

  operation, format        | slack needed       | constant | worst distance from the box | allowance            | share judged
  warp u8c3 / u8c1 / u8c4  | 0                  | 0        | 0.501 LSB                   | 1 (the project's bar)| homography >= 0.991,
  warp u16c3               | 1 ulp (1080p noise;| 2 ulp    | 0.496 LSB                   | 0.5 + 10 * 2^-9      |  1080p 0.998; mesh 0.859
                           |  1/8 ulp up to 640) |          |                             |  = 0.5195            |  (required 0.97 / 0.60)
  resize u8c3 / u8c1 / u8c4| 0                  | 0        | 0.818 LSB                   | 1                    | 1.0
  resize u16c3             | 1/2 ulp (<= 640 and| 1 ulp    | 0.504 LSB                   | 0.5195               | 1.0
                           |  1080p alike)      |          |                             |                      |
  warp u8c2 (NV12 chroma) | 0                  | 0        | 0.500 LSB                   | 1                    | homography >= 0.993,
  warp u16c2 (P010 chroma) | 1/2 ulp (1080p     | 2 ulp    | 0.489 LSB                   | 0.5195 (the same ten |  1080p 0.997, odd shifts
                           |  noise, 32 x 32    |          |                             |  roundings, counted  |  0.996, 1/32 shift 0.989;
                           |  mesh; 1/4 ulp on  |          |                             |  at VALUE_ALLOW)     |  mesh 0.859
                           |  16 x 16; 0 <= 640)|          |                             |                      |
  resize u8c2              | 0                  | 0        | 0.813 LSB                   | 1                    | 1.0
  resize u16c2             | 1/2 ulp (<= 640 and| 1 ulp    | 0.505 LSB (0.519 at 1/2 ulp)| 0.5195               | 1.0
                           |  1080p alike)      |          |                             |                      |
  The chroma rows were measured on WARP_CASES_420 plus both 1080p homographies, and on RESIZE_CASES_420 plus the 1080p and same-size
  cases, against tests/nv12_model.py, p010_model.py, nv12_crop_model.py and p010_crop_model.py alone; ulps are counted at the chroma
  plane's extent (the resize positions are absolute in that plane).  Distances at slack 0 on 1080p noise: warp 0.81 LSB (16 x 16 mesh) and
  1.62 LSB (32 x 32) from the box, resize 2.97 LSB.  The warp constant is u16c3's by derivation, not by the ladder (which would give 1 ulp):
  the chroma maps are the luma maps halved exactly and the chroma extent's ulp is half the luma extent's, so the same half ulp of the map
  and half ulp of the vertices arrive, counted in the same unit.  Chroma mean signed difference (P010, smooth, two frames shifted by
  (6 14/32, -2 22/32), 130,140 values): +0.00019 LSB; truncation moves it to -0.50.
  2 ulp at 1080p is 2^-12 px, far below the caps (1/64 px warp, 2^-10 px resize) beyond which a bucket taken by floor would pass.
  The uint16 allowance is derived, not measured: 0.5 for the final rounding and ten float32 roundings of values below 65,536 (half an ulp,
  2^-9, each: seven in the remap's four products and three sums, nine in the resize's two passes and its 1 - f) -- the measurement agrees.
  Why 1 ulp for the warp: half an ulp from rounding the map to float32 and up to half an ulp from the float32 vertices the homography is
  solved from.  It shows at 1080p (coordinates above 1024) on noise only; on frames up to 640 wide one value of 1.4 million needed any.
  Mean signed difference (uint16, smooth frames, >= 100,000 values): the rounding error is uniform in +-0.5, standard deviation 1/sqrt(12),
  so 3 standard errors at 100,000 values are 0.00274 LSB.  Measured: warp shifted by (5 7/32, -3 11/32) -0.00024; resize cases 11, 18, 19
  and the same-size ones -0.00023, -0.00019, -0.00011, -0.00013, -0.00028.  Truncation moves it to -0.49.

The values that fell outside the first cross-check's envelope (nine fixed points at +-1/64 px, 1 LSB) on uint16, 270 x 484, 5 x 7 mesh, one
global homography, classified:

  frames                  | outside            | where                                        | an integer line crosses the box
  smooth, times 257       | 8-18 values, <= 9.2| all but one within a pixel of the frame's edge| all
  uniform noise           | 1.5-2 % of pixels, | of them 1 % at the edge, 8 % on cell seams,  | all
                          |  <= 558 LSB        |  the rest in cell interiors                  |

  Every one is a fault of that envelope, none of the model: the sample is piecewise bilinear, and where a source cell boundary crosses
  the box its extreme lies on that line, between the nine points (at the frame's edge the kink against the border is the largest there
  is).  With the exact envelope no value is left outside on these frames at slack 0, and the models were left alone.

What this cannot tell apart.  The exact-2x uint16 area branch and the float path differ only in how an exact .5 is rounded (half up against
half to even): both lie within 0.5 LSB of the float64 value, so the envelope passes either, and although their means differ by 1/8 LSB no
float64 sampler can say which of the two OpenCV takes -- that case is left out of the mean check and the branch stays unchecked here.
Nor can it see the last bit of the 8-bit fixed-point paths (1 LSB allowance), the painter order on cell seams (mesh cases judge cell
interiors only), or who paints the one-pixel ring outside the frame's edge.
For 4:2:0 chroma it cannot see who owns the ring either, and that ring is wider: a chroma sample whose siting luma pixel has its source
outside the frame may be the border outright or a blend, anywhere within one chroma pixel (two luma pixels) of the plane's edge
(`chroma_ring`); under a shift by (5 7/32, -3 11/32) every chroma coordinate is a tie of the 1/32 bucket, so which way cvRound breaks ties
is invisible to the envelope there and the chroma mean is taken on a sixteenths shift instead.  In the crop-resize the x axis zeroes its
fraction where it clamps and the y axis keeps it on two rows clipped to one: both are the value at the clamped position, so which of the
two a kernel does cannot be told, nor should it.  A clamp range one sample too wide shows only where the extra sample differs (noise, or
a steep frame) and only in the one or two edge samples that clamp (on 8-bit smooth frames by 0.8 LSB: noise is the case that counts).
Every wrong 4:2:0 model of tests/test_second_opinion_models.py is rejected; none had to be listed here.
"""
import collections
import math

import numpy as np
import torch

F_ = torch.nn.functional

FORMATS = ('u8c3', 'u16c3', 'u8c1', 'u8c4')
CHANNELS = {'u8c3': 3, 'u16c3': 3, 'u8c1': 1, 'u8c4': 4}
TOP = {'u8c3': 255, 'u16c3': 65535, 'u8c1': 255, 'u8c4': 255}
# 4:2:0: a luma plane and an interleaved (U, V) plane of half the size in each axis, each judged as a format of its own.  NV12 luma is the
# u8c1 launch; P010 luma is channel 0 of u16c3 bit for bit, so it is a one-channel plane with u16c3's constants (the arithmetic is per channel)
FORMATS_420 = ('nv12', 'p010')
LUMA_OF = {'nv12': 'u8c1', 'p010': 'u16c1'}
CHROMA_OF = {'nv12': 'u8c2', 'p010': 'u16c2'}
CHANNELS.update({'u16c1': 1, 'u8c2': 2, 'u16c2': 2})
TOP.update({'u16c1': 65535, 'u8c2': 255, 'u16c2': 65535})

# ---- the constants (how each was fixed: the table above) ------------------------------------------------------------------------------

BUCKET = 1.0 / 64                    # coordinate half-width of cv2.remap's 1/32-pixel bucket, px
# float32 coordinate slack, in float32 ulps of the largest source coordinate of the case (`coordinate_ulp`): twice the measured need
WARP_EPS_ULPS = {'u8c3': 0.0, 'u16c3': 2.0, 'u8c1': 0.0, 'u8c4': 0.0}
RESIZE_EPS_ULPS = {'u8c3': 0.0, 'u16c3': 1.0, 'u8c1': 0.0, 'u8c4': 0.0}
WARP_EPS_CAP = 1.0 / 64              # px: a slack beyond these could no longer reject a coordinate bucket taken by floor
RESIZE_EPS_CAP = 2.0 ** -10
HALF_ULP_U16 = 2.0 ** -9             # half a float32 ulp of a value in [32768, 65536)
VALUE_ALLOW = {'u8c3': 1.0, 'u16c3': 0.5 + 10 * HALF_ULP_U16, 'u8c1': 1.0, 'u8c4': 1.0}             # LSB of the format
# the chroma planes (the table's 4:2:0 rows; ulps are counted at the chroma plane's extent) and P010 luma (u16c3's, per channel).  The
# u16c2 allowance is u16c3's because the count is: the warp is cv16_model.remap_bilinear_u16c3 itself (seven roundings), and
# p010_crop_model.blend rounds three times per horizontal tap pair (two products, one sum), three times in the vertical pass, and once in
# each 1 - f that reaches a value -- ten at the most
WARP_EPS_ULPS.update({'u16c1': WARP_EPS_ULPS['u16c3'], 'u8c2': 0.0, 'u16c2': 2.0})
RESIZE_EPS_ULPS.update({'u16c1': RESIZE_EPS_ULPS['u16c3'], 'u8c2': 0.0, 'u16c2': 1.0})
VALUE_ALLOW.update({'u16c1': VALUE_ALLOW['u16c3'], 'u8c2': 1.0, 'u16c2': 0.5 + 10 * HALF_ULP_U16})
MEAN_SIGNED_VALUES = 100000         # the mean signed difference is judged on at least this many values
MEAN_SIGNED_BOUND = 3 * math.sqrt(1.0 / 12) / math.sqrt(MEAN_SIGNED_VALUES)                         # 3 standard errors: 0.00274 LSB
SHARE_GLOBAL = 0.97                  # global-homography and resize cases judge at least this share of their pixels
SHARE_MESH = 0.60                    # mesh-motion cases (cell interiors only)
EXACT = 1e-6                         # identity and integer shifts: grid_sample's normalised coordinates return an integer as integer +- 1e-13

# ---- the case table ---------------------------------------------------------------------------------------------------------------------

WarpCase = collections.namedtuple('WarpCase', 'kind n H W R C seed')
# kind: 'identity', 'shift' (two integer shifts), 'homography' (one global homography per frame), 'mesh' (every cell its own), 'far'
# (a large shift: a wide uncovered band for the border checks), 'thirtyseconds' (a shift by multiples of 1/32 px: no bucket error, the
# difference from the centre sample is the rounding of the value alone -- the mean-signed-difference case)
WARP_CASES = [
    WarpCase('identity', 2, 270, 484, 5, 7, 0),
    WarpCase('shift', 2, 270, 484, 5, 7, 0),
    WarpCase('shift', 2, 360, 640, 16, 16, 0),
    WarpCase('homography', 2, 270, 484, 5, 7, 2),
    WarpCase('homography', 2, 360, 640, 16, 16, 1),
    WarpCase('mesh', 2, 360, 640, 8, 8, 5),
    WarpCase('far', 1, 270, 484, 5, 7, 6),
    WarpCase('thirtyseconds', 1, 270, 484, 5, 7, 7),
]
WARP_CASES_1080P = [                 # on the CPU for u16c3 only (the one format whose slack is not 0), on the GPU for every format
    WarpCase('homography', 1, 1080, 1920, 16, 16, 3),
    WarpCase('homography', 1, 1080, 1920, 32, 32, 4),
    WarpCase('shift', 1, 1080, 1920, 16, 16, 0),
]
INTEGER_SHIFTS = ((5, -3), (-4, 6))
FAR_SHIFT = (37, -29)
THIRTYSECONDS_SHIFT = (5 + 7 / 32, -3 - 11 / 32)

# (n, H, W, rect, (out_W, out_H)): tests/test_gpu_crop_resize_to.py's CASES, restated (that module imports the package at load)
RESIZE_CASES = [
    (3, 48, 64, (5, 3, 40, 30), (90, 70)),            # upscale, non-integer ratios
    (3, 120, 200, (3, 5, 190, 110), (61, 37)),        # downscale, non-integer
    (2, 160, 96, (10, 10, 50, 150), (120, 40)),       # up in x, down in y
    (2, 96, 160, (10, 10, 150, 50), (40, 120)),       # down in x, up in y
    (3, 90, 130, (1, 3, 120, 82), (60, 40)),          # exactly 2x down (u16: INTER_AREA's fast path)
    (2, 95, 127, (2, 1, 121, 90), (40, 30)),          # exactly 3x down
    (2, 33, 47, (4, 2, 40, 30), (1, 1)),              # 1 x 1 output
    (2, 33, 47, (4, 2, 40, 30), (1, 37)),             # 1 x N
    (2, 33, 47, (4, 2, 40, 30), (29, 1)),             # N x 1
    (2, 21, 19, (5, 7, 5, 7), (17, 9)),               # 1-pixel crop
    (2, 21, 19, (0, 7, 18, 7), (13, 5)),              # 1-row crop, down in x
    (2, 30, 41, (0, 0, 40, 29), (301, 203)),          # output larger than the frame
    (2, 31, 67, (3, 2, 66, 30), (129, 61)),           # W % 4 != 0 in and out
    (2, 40, 700, (20, 0, 619, 39), (250, 20)),        # 2.4x in x: u8c3 staged
    (2, 40, 1000, (10, 0, 684, 39), (250, 20)),       # 2.7x in x: just above the u8c3 cut-over
    (2, 40, 900, (20, 0, 819, 39), (250, 20)),        # 3.2x in x: u8c3 direct, u8c1 staged
    (2, 40, 1400, (20, 0, 1269, 39), (250, 20)),      # 5x in x: both direct
    (1, 300, 1000, (0, 0, 999, 299), (97, 29)),       # ~10x down in both axes
    (20, 64, 300, (7, 5, 290, 60), (700, 90)),        # many frames and tiles (XCD tile order), up
    (20, 300, 520, (7, 5, 510, 290), (170, 150)),     # many frames, down
]
RESIZE_CASES_1080P = [               # 1080p, one downscale on each side of each staged / direct cut-over: CPU for u16c3, GPU for all
    (1, 1080, 1920, (17, 9, 1899, 1071), (1280, 720)),    # 1.47x down: every format staged
    (1, 1080, 1920, (0, 0, 1919, 1079), (960, 540)),      # exactly 2x (u16: the area branch)
    (1, 1080, 1920, (10, 4, 1909, 1075), (810, 456)),     # 2.35x: below u8c4's cut-over (2.37)
    (1, 1080, 1920, (10, 4, 1909, 1075), (780, 440)),     # 2.44x: above u8c4's, below u8c3's (2.64)
    (1, 1080, 1920, (10, 4, 1909, 1075), (700, 394)),     # 2.71x: above u8c3's, below u8c1's (3.99)
    (1, 1080, 1920, (10, 4, 1909, 1075), (470, 264)),     # 4.04x: above u8c1's: every format direct
]
SAME_SIZE_CASES = [                  # (n, H, W, rect): the call without `size` (back to the frame size), today's rectangles
    (2, 360, 640, (13, 11, 629, 350)),
    (2, 270, 484, (0, 0, 483, 269)),
    (2, 270, 484, (40, 30, 443, 239)),
]
SAME_SIZE_CASES_1080P = [(1, 1080, 1920, (17, 9, 1899, 1071))]

# a non-black border per format; u16c3: the default, which must come out as 255, not 65,535
BORDERS = {'u8c3': (11, 122, 233), 'u16c3': (0, 0, 255), 'u8c1': (77,), 'u8c4': (11, 122, 233, 44)}

# ---- the 4:2:0 case table -----------------------------------------------------------------------------------------------------------------

BORDERS_YUV = {'nv12': (19, 203, 77), 'p010': (4921, 52107, 19733)}      # (Y, U, V), all three different: a border from the wrong component shows
# a shift by multiples of 1/16 luma px: halved it is a multiple of 1/32 chroma px, so chroma has no bucket error either (THIRTYSECONDS_SHIFT
# halves to odd multiples of 1/64 chroma px, every one a rounding tie of the bucket: the true P010 chroma mean comes out at -0.25 LSB there)
SIXTEENTHS_SHIFT = (6 + 14 / 32, -2 - 22 / 32)
# the warp cases (every size is even already) and the chroma mean-signed case: two frames, 65,340 chroma values each
WARP_CASES_420 = WARP_CASES + [WarpCase('sixteenths', 2, 270, 484, 5, 7, 8)]


def _even(v):
    return v + v % 2


def _resize_cases_420():
    """RESIZE_CASES with the frame and the output made even (odd numbers go up by one; the rectangle stays) and at most two frames; a
    100 x 72 frame with both parities of every edge of the rectangle; one-pixel crops on an odd column and row and on the frame's last pixel."""
    cases = [(min(n, 2), _even(H), _even(W), rect, (_even(ow), _even(oh))) for n, H, W, rect, (ow, oh) in RESIZE_CASES]
    for k in range(16):
        rect = (10 + (k & 1), 6 + (k >> 1 & 1), 80 + (k >> 2 & 1), 60 + (k >> 3 & 1))
        cases.append((1, 72, 100, rect, ((46, 90)[k & 1], (34, 80)[k >> 1 & 1])))      # down and up, non-integer ratios
    cases += [(2, 72, 100, (37, 21, 37, 21), (18, 10)), (2, 72, 100, (99, 71, 99, 71), (6, 4)), (2, 72, 100, (98, 70, 99, 71), (10, 8)),
              (2, 72, 100, (0, 0, 99, 71), (100, 72))]                    # ..., the last 2 x 2 pixels, the whole frame at its own size
    return cases


RESIZE_CASES_420 = _resize_cases_420()
PARITY_CASE_420 = next(c for c in RESIZE_CASES_420 if c[1:3] == (72, 100) and c[3][0] % 2 and c[3][1] % 2)   # odd left, odd top


# ---- frames ---------------------------------------------------------------------------------------------------------------------------

def smooth_planes(fmt, n, H, W, seed=0, device='cpu'):
    """Band-limited frames (sums of sinusoids, gradients of about 3/256 of the range per pixel) as float64 planes (n, H, W, channels) of
    integer values in 0 .. TOP[fmt].  Every channel has its own phase, alpha included; uint16 takes the full range (not multiples of 257).
    u8c3 frames are those of this project's first torch cross-check, byte for byte."""
    ch, s = CHANNELS[fmt], (TOP[fmt] + 1) / 256
    y = torch.arange(H, dtype=torch.float64, device=device)[None, :, None, None]
    x = torch.arange(W, dtype=torch.float64, device=device)[None, None, :, None]
    c = torch.arange(ch, dtype=torch.float64, device=device)[None, None, None, :]
    f = torch.arange(n, dtype=torch.float64, device=device)[:, None, None, None] + seed
    v = 128 + 60 * torch.sin(0.031 * x + 0.017 * y + 0.7 * c + 0.3 * f) + 50 * torch.cos(0.011 * x - 0.043 * y + 1.3 * c - 0.2 * f)
    return (v * s).round().clamp(0, TOP[fmt])


def noise_planes(fmt, n, H, W, seed=0, device='cpu'):
    """Uniform noise over the full range (drawn on the CPU, so the same values on every device)."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(0, TOP[fmt] + 1, (n, H, W, CHANNELS[fmt]), generator=g).to(torch.float64).to(device)


def to_numpy(fmt, planes):
    """Planes -> the NumPy stack a model takes: (n, H, W, 2, 3 or 4) uint8 / uint16, or (n, H, W) for one channel."""
    a = planes.cpu().numpy().astype(np.uint16 if TOP[fmt] > 255 else np.uint8)
    return a[..., 0] if CHANNELS[fmt] == 1 else a


def to_planes(a, device='cpu'):
    """A model's NumPy result -> float64 planes (n, H, W, channels)."""
    t = torch.from_numpy(np.ascontiguousarray(a).astype(np.float64)).to(device)
    return t[..., None] if t.dim() == 3 else t


def border_planes(fmt, border, device='cpu'):
    """The border as OpenCV applies it: the components themselves (not scaled to 16 bits), missing ones 0 (cv::Scalar's padding)."""
    b = [float(min(max(round(c), 0), TOP[fmt])) for c in border][:CHANNELS[fmt]]
    return torch.tensor(b + [0.0] * (CHANNELS[fmt] - len(b)), dtype=torch.float64, device=device)


# ---- coordinate maps, float64 ---------------------------------------------------------------------------------------------------------

def grid(W, H, R, C):
    """Mesh vertex pixel positions: ceil((W-1) col / C), ceil((H-1) row / R)."""
    gx = np.array([np.ceil((W - 1) * (c / C)) for c in range(C + 1)])
    gy = np.array([np.ceil((H - 1) * (r / R)) for r in range(R + 1)])
    return gx, gy


def pixels(n, H, W, device='cpu'):
    ys = torch.arange(H, dtype=torch.float64, device=device)[None, :, None].expand(n, H, W)
    xs = torch.arange(W, dtype=torch.float64, device=device)[None, None, :].expand(n, H, W)
    return xs, ys


def homography_motion(n, H, W, R, C, seed):
    """Every vertex moved by one global homography G per frame (rotation, shear, perspective, sub-pixel shift).
    Returns (unstab, stab (n, R+1, C+1, 2) float64, G (n, 3, 3))."""
    rng = np.random.RandomState(seed)
    gx, gy = grid(W, H, R, C)
    unstab = np.zeros((n, R + 1, C + 1, 2))
    stab = np.zeros_like(unstab)
    Gs = []
    for f in range(n):
        a = rng.uniform(-0.01, 0.01)
        G = np.array([[np.cos(a) * (1 + rng.uniform(-0.01, 0.01)), -np.sin(a) + rng.uniform(-0.004, 0.004), rng.uniform(-6, 6)],
                      [np.sin(a), np.cos(a) * (1 + rng.uniform(-0.01, 0.01)), rng.uniform(-6, 6)],
                      [rng.uniform(-4e-6, 4e-6), rng.uniform(-4e-6, 4e-6), 1.0]])
        Gs.append(G)
        X, Y = np.meshgrid(gx, gy)
        w = G[2, 0] * X + G[2, 1] * Y + G[2, 2]
        stab[f, :, :, 0] = (G[0, 0] * X + G[0, 1] * Y + G[0, 2]) / w - X
        stab[f, :, :, 1] = (G[1, 0] * X + G[1, 1] * Y + G[1, 2]) / w - Y
    return unstab, stab, np.stack(Gs)


def shift_motion(n, R, C, dx, dy):
    z = np.zeros((n, R + 1, C + 1, 2))
    s = z.copy()
    s[..., 0] = dx
    s[..., 1] = dy
    return z, s


def mesh_motion(n, R, C, seed):
    """Smooth per-vertex motion, every cell its own homography: a translation plus two low-frequency waves of 1.5 px."""
    rng = np.random.RandomState(seed)
    rr = np.arange(R + 1)[None, :, None] / R
    cc = np.arange(C + 1)[None, None, :] / C
    unstab = np.zeros((n, R + 1, C + 1, 2))
    stab = np.zeros_like(unstab)
    for k in range(2):
        t = rng.uniform(-3, 3, (n, 1, 1))
        ph = rng.uniform(0, 2 * np.pi, (2, n, 1, 1))
        fr = rng.uniform(0.5, 1.5, (2, n, 1, 1))
        stab[..., k] = t + 1.5 * np.cos(2 * np.pi * (fr[0] * rr + 0.7 * cc) + ph[0]) + 1.5 * np.sin(2 * np.pi * (0.6 * rr + fr[1] * cc) + ph[1])
    return unstab, stab


def source_map(M, n, H, W, device='cpu'):
    """(u, v) = M x for every output pixel x, M (n, 3, 3) float64: the source position of each output pixel when M = G^-1."""
    xs, ys = pixels(n, H, W, device)
    M = torch.as_tensor(M, dtype=torch.float64, device=device)
    g = lambda i, j: M[:, i, j][:, None, None]                           # noqa: E731
    w = g(2, 0) * xs + g(2, 1) * ys + g(2, 2)
    return (g(0, 0) * xs + g(0, 1) * ys + g(0, 2)) / w, (g(1, 0) * xs + g(1, 1) * ys + g(1, 2)) / w


def inverse(G, device='cpu'):
    return torch.linalg.inv(torch.as_tensor(G, dtype=torch.float64, device=device))


def border_ring(u, v, H, W):
    """Output pixels whose source lies within 1.5 pixels outside the frame: between the frame's edge and the edge of the warped mesh the
    reference's cell masks decide whether a pixel is painted at all (the border colour where not), which a sampler of the frame alone
    cannot know."""
    return ((u < 0) & (u > -1.5)) | ((u > W - 1) & (u < W + 0.5)) | ((v < 0) & (v > -1.5)) | ((v > H - 1) & (v < H + 0.5))


def far_outside(u, v, H, W):
    """Output pixels whose source lies well outside the frame: the border value exactly."""
    return (u < -2) | (u > W + 1) | (v < -2) | (v > H + 1)


def mesh_interior_map(H, W, R, C, unstab_f, stab_f, device='cpu'):
    """Real mesh motion of one frame: per cell the exact 4-point homography (stabilized corners -> grid corners) is solved here with
    torch.linalg.solve; every output pixel that lies inside the stabilized quad of exactly one cell, two pixels away from its edges, takes
    that cell's map.  Returns (u, v, sure), each (H, W); u, v are 0 where not sure.  (Pixels near cell borders are owned by the
    reference's painter order -- pinned by the goldens, not judged here.)"""
    gx, gy = grid(W, H, R, C)
    xs, ys = pixels(1, H, W, device)
    xs, ys = xs[0], ys[0]
    u = torch.full((H, W), float('nan'), dtype=torch.float64, device=device)
    v = torch.full_like(u, float('nan'))
    owners = torch.zeros((H, W), dtype=torch.int32, device=device)
    P = np.stack(np.meshgrid(gx, gy), axis=-1) + (np.asarray(stab_f) - np.asarray(unstab_f))       # stabilized vertex positions
    for r in range(R):
        for c in range(C):
            src = np.array([P[r, c], P[r, c + 1], P[r + 1, c], P[r + 1, c + 1]]).astype(np.float32).astype(np.float64)
            dst = np.array([[gx[c], gy[r]], [gx[c + 1], gy[r]], [gx[c], gy[r + 1]], [gx[c + 1], gy[r + 1]]])
            A, b = [], []
            for (x, y), (X, Y) in zip(src, dst):                         # h maps (x, y) -> (X, Y), h22 = 1
                A.append([x, y, 1, 0, 0, 0, -X * x, -X * y]); b.append(X)
                A.append([0, 0, 0, x, y, 1, -Y * x, -Y * y]); b.append(Y)
            h = torch.linalg.solve(torch.tensor(A, dtype=torch.float64), torch.tensor(b, dtype=torch.float64))
            h = [float(t) for t in h] + [1.0]
            w = h[6] * xs + h[7] * ys + h[8]
            uu = (h[0] * xs + h[1] * ys + h[2]) / w
            vv = (h[3] * xs + h[4] * ys + h[5]) / w
            inside = (uu > gx[c] + 2) & (uu < gx[c + 1] - 2) & (vv > gy[r] + 2) & (vv < gy[r + 1] - 2)
            loose = (uu > gx[c] - 2) & (uu < gx[c + 1] + 2) & (vv > gy[r] - 2) & (vv < gy[r + 1] + 2)
            owners += loose.to(torch.int32)
            u = torch.where(inside, uu, u)
            v = torch.where(inside, vv, v)
    sure = ~torch.isnan(u) & (owners == 1)
    return torch.where(sure, u, torch.zeros_like(u)), torch.where(sure, v, torch.zeros_like(v)), sure


# ---- the references -------------------------------------------------------------------------------------------------------------------

def coordinate_ulp(extent):
    """The float32 ulp of the largest coordinate of a source `extent` samples long, px: 2^-14 for 513 .. 1024, 2^-13 up to 2048."""
    return 2.0 ** (math.floor(math.log2(max(extent - 1, 1))) - 23)


def warp_eps(fmt, H, W, ulps=None):
    eps = (WARP_EPS_ULPS[fmt] if ulps is None else ulps) * coordinate_ulp(max(H, W))
    assert eps <= WARP_EPS_CAP
    return eps


def resize_eps(fmt, crop_h, crop_w, ulps=None):
    eps = (RESIZE_EPS_ULPS[fmt] if ulps is None else ulps) * coordinate_ulp(max(crop_h, crop_w))
    assert eps <= RESIZE_EPS_CAP
    return eps


def sample(planes, u, v, border=None, clamp=False):
    """grid_sample (bilinear, align_corners=True: pixel centres at integers) of float64 planes (n, H, W, ch) at source positions u, v
    (n, h, w) in PIXEL units -> (n, h, w, ch).  Taps outside the frame take the border value of their channel (`border`: (ch,) tensor,
    None = 0): the planes are sampled minus the border with zero padding and the border is added back.  clamp=True: positions are
    clamped to the frame instead (the resize's edge rule)."""
    n, H, W, _ = planes.shape
    src = planes if border is None else planes - border
    src = src.permute(0, 3, 1, 2)
    gx = 2 * u / (W - 1) - 1 if W > 1 else torch.zeros_like(u)          # -1 <-> pixel 0, +1 <-> pixel W-1
    gy = 2 * v / (H - 1) - 1 if H > 1 else torch.zeros_like(v)
    out = F_.grid_sample(src, torch.stack([gx, gy], dim=-1), mode='bilinear', padding_mode='border' if clamp else 'zeros',
                         align_corners=True).permute(0, 2, 3, 1)
    return out if border is None else out + border


def interpolate(planes, out_w, out_h):
    """The resize reference: bilinear, half-pixel centres (align_corners=False), no antialiasing, float64."""
    return F_.interpolate(planes.permute(0, 3, 1, 2), size=(out_h, out_w), mode='bilinear', align_corners=False,
                          antialias=False).permute(0, 2, 3, 1)


def resize_positions(src_len, dst_len, device='cpu'):
    """The exact source position of every output sample: (d + 0.5) src / dst - 0.5, clamped to the crop."""
    d = torch.arange(dst_len, dtype=torch.float64, device=device)
    return ((d + 0.5) * (src_len / dst_len) - 0.5).clamp(0, src_len - 1)


def _box_points(p, half):
    """Three positions per value that carry the extremes of a piecewise-linear function over [p - half, p + half] (half < 0.5): the two
    ends, and the integer line that crosses the interval where one does (the centre where none does)."""
    k = p.round()
    return p - half, torch.where((k - p).abs() < half, k, p), p + half


def envelope(planes, u, v, half, border=None, clamp=False, lim=None):
    """(lo, hi): the range the bilinear sample takes over the box [u +- half] x [v +- half].  The sample is bilinear inside each source
    cell, so on every piece of the box its extremes sit at the piece's corners: the box's own corners and, where an integer line crosses
    it, the points on that line -- 3 x 3 samples, exact for half < 0.5, nothing missed between them.  clamp: the box is clamped to the
    plane, or to `lim` = ((x0, x1), (y0, y1)) inside it."""
    if clamp and lim is None:
        lim = ((0, planes.shape[2] - 1), (0, planes.shape[1] - 1))
    lo = hi = None
    for pu in _box_points(u, half):
        for pv in _box_points(v, half):
            if clamp:
                pu, pv = pu.clamp(*lim[0]), pv.clamp(*lim[1])
            s = sample(planes, pu, pv, border, clamp)
            lo = s if lo is None else torch.minimum(lo, s)
            hi = s if hi is None else torch.maximum(hi, s)
    return lo, hi


Verdict = collections.namedtuple('Verdict', 'excess worst share mean_signed values')


def judge(got, centre, lo, hi, allow, judged=None):
    """Numbers, no assertion.  got, centre, lo, hi: float64 (n, h, w, ch); judged: bool (n, h, w) or None (all).
    excess: per value, how far it lies outside [lo - allow, hi + allow] (0 inside, 0 where not judged); worst: its maximum; share: the
    share of pixels judged; mean_signed: the mean of got - centre over the judged values; values: how many were judged."""
    excess = torch.maximum(torch.maximum(lo - allow - got, got - hi - allow), torch.zeros_like(got))
    diff = got - centre
    if judged is not None:
        excess = excess * judged[..., None]
        diff = diff[judged]
    values = diff.numel()
    return Verdict(excess, float(excess.max()) if excess.numel() else 0.0, 1.0 if judged is None else float(judged.double().mean()),
                   float(diff.mean()) if values else 0.0, values)


def judge_warp(fmt, got, planes, u, v, border, judged=None, eps=None, allow=None):
    """The warp's verdict: envelope = the coordinate half-width BUCKET + warp_eps around (u, v), value allowance VALUE_ALLOW[fmt].
    eps: the slack in ulps instead of WARP_EPS_ULPS[fmt] (for measuring)."""
    half = BUCKET + warp_eps(fmt, planes.shape[1], planes.shape[2], eps)
    b = border_planes(fmt, border, planes.device)
    lo, hi = envelope(planes, u, v, half, b)
    return judge(got, sample(planes, u, v, b), lo, hi, VALUE_ALLOW[fmt] if allow is None else allow, judged)


def far_mismatches(fmt, got, u, v, border, far=None):
    """(values well outside the frame that are not the border value exactly, number of such pixels)."""
    H, W = got.shape[1:3]
    far = far_outside(u, v, H, W) if far is None else far
    return int((got[far] != border_planes(fmt, border, got.device)).sum()), int(far.sum())


def judge_resize(fmt, got, planes, rect, out_w, out_h, eps=None, allow=None):
    """The crop-resize's verdict: the centre is `interpolate` of the crop; the envelope is resize_eps around the exact source position
    (sampled by grid_sample clamped to the crop, which must agree with interpolate at the centre: also returned, as `agree`)."""
    left, top, right, bottom = rect
    crop = planes[:, top:bottom + 1, left:right + 1]
    n = crop.shape[0]
    centre = interpolate(crop, out_w, out_h)
    u = resize_positions(crop.shape[2], out_w, crop.device)[None, None, :].expand(n, out_h, out_w)
    v = resize_positions(crop.shape[1], out_h, crop.device)[None, :, None].expand(n, out_h, out_w)
    lo, hi = envelope(crop, u, v, resize_eps(fmt, crop.shape[1], crop.shape[2], eps), None, clamp=True)
    agree = float((sample(crop, u, v, None, clamp=True) - centre).abs().max())
    lo, hi = torch.minimum(lo, centre), torch.maximum(hi, centre)
    return judge(got, centre, lo, hi, VALUE_ALLOW[fmt] if allow is None else allow), agree


def legacy_assert_within_envelope(got, frames, u, v, allow=1.0, skip=None):
    """The first cross-check's assertion, kept for its tests: got (uint8) within `allow` + 0.5 grey levels of the range the float64 sample
    of uint8 frames (n, H, W, 3) takes at the nine points of the 1/32-pixel bucket around (u, v).  Returns mean |got - centre|."""
    planes = frames.to(torch.float64)
    lo = hi = None
    for du in (-1 / 64, 0.0, 1 / 64):
        for dv in (-1 / 64, 0.0, 1 / 64):
            s = sample(planes, u + du, v + dv)
            lo = s if lo is None else torch.minimum(lo, s)
            hi = s if hi is None else torch.maximum(hi, s)
    g = got.to(torch.float64)
    bad = (g < lo - allow - 0.5) | (g > hi + allow + 0.5)                           # (+0.5: rounding of the final value)
    if skip is not None:
        bad = bad & ~skip[..., None]
    assert not bool(bad.any()), f'{int(bad.sum())} of {bad.numel()} values outside the envelope; worst {float(torch.maximum(lo - g, g - hi).max()):.2f}'
    return float((g - sample(planes, u, v)).abs().mean())


# ---- cases -> what to judge -----------------------------------------------------------------------------------------------------------

# far: which samples must be the border exactly (None: `far_outside` of (u, v))
WarpSetup = collections.namedtuple('WarpSetup', 'label unstab stab u v judged exact min_share far', defaults=(None,))


def warp_setups(case, device='cpu'):
    """The mesh motions of one case and, for each, the float64 source map, which pixels are judged, and whether the answer is exact."""
    n, H, W, R, C = case.n, case.H, case.W, case.R, case.C
    xs, ys = pixels(n, H, W, device)
    if case.kind in ('identity', 'shift', 'far'):
        shifts = {'identity': ((0, 0),), 'shift': INTEGER_SHIFTS, 'far': (FAR_SHIFT,)}[case.kind]
        for dx, dy in shifts:                                           # content moves by (+dx, +dy): the map is (x - dx, y - dy)
            unstab, stab = shift_motion(n, R, C, dx, dy)
            yield WarpSetup(f'{case.kind}{(dx, dy)}', unstab, stab, xs - dx, ys - dy, None, True, 1.0)
    elif case.kind in ('thirtyseconds', 'sixteenths'):
        dx, dy = THIRTYSECONDS_SHIFT if case.kind == 'thirtyseconds' else SIXTEENTHS_SHIFT
        unstab, stab = shift_motion(n, R, C, dx, dy)
        u, v = xs - dx, ys - dy
        yield WarpSetup(case.kind, unstab, stab, u, v, ~border_ring(u, v, H, W), False, SHARE_GLOBAL)
    elif case.kind == 'homography':
        unstab, stab, G = homography_motion(n, H, W, R, C, case.seed)
        u, v = source_map(inverse(G, device), n, H, W, device)
        yield WarpSetup('homography', unstab, stab, u, v, ~border_ring(u, v, H, W), False, SHARE_GLOBAL)
    elif case.kind == 'mesh':
        unstab, stab = mesh_motion(n, R, C, case.seed)
        maps = [mesh_interior_map(H, W, R, C, unstab[f], stab[f], device) for f in range(n)]
        u, v, sure = (torch.stack([m[k] for m in maps]) for k in range(3))
        yield WarpSetup('mesh', unstab, stab, u, v, sure, False, SHARE_MESH)
    else:
        raise ValueError(case.kind)


def warp_findings(fmt, got, planes, setup, border, eps=None, allow=None):
    """The numbers of one warp result `got` (float64 planes): worst (exact setups: max |got - sample|; else the worst excess over the
    envelope), share, mean_signed, values, and far_bad / far_pixels (values far outside the frame that are not the border exactly)."""
    if setup.exact:
        diff = got - sample(planes, setup.u, setup.v, border_planes(fmt, border, planes.device))
        worst, share, mean_signed, values = float(diff.abs().max()), 1.0, float(diff.mean()), diff.numel()
    else:
        vd = judge_warp(fmt, got, planes, setup.u, setup.v, border, setup.judged, eps, allow)
        worst, share, mean_signed, values = vd.worst, vd.share, vd.mean_signed, vd.values
    far_bad, far_pixels = far_mismatches(fmt, got, setup.u, setup.v, border, setup.far)
    return dict(label=setup.label, worst=worst, share=share, mean_signed=mean_signed, values=values, far_bad=far_bad, far_pixels=far_pixels)


def warp_violations(fmt, f, setup, smooth):
    """What of the findings `f` breaks the contract, as a list of sentences (empty: inside)."""
    out = []
    if setup.exact and f['worst'] >= EXACT:
        out.append(f"{f['label']}: not the shifted frame itself, worst difference {f['worst']:.3g}")
    if not setup.exact and f['worst'] > 0:
        out.append(f"{f['label']}: {f['worst']:.3f} LSB outside the envelope")
    if f['share'] < setup.min_share:
        out.append(f"{f['label']}: only {f['share']:.3f} of the pixels judged, {setup.min_share} required")
    if f['far_bad']:
        out.append(f"{f['label']}: {f['far_bad']} values far outside the frame are not the border value")
    if setup.label.startswith('far') and not f['far_pixels']:
        out.append(f"{f['label']}: no pixel far outside the frame")
    if smooth and TOP[fmt] == 65535 and setup.label == ('sixteenths' if CHANNELS[fmt] == 2 else 'thirtyseconds'):
        if f['values'] < MEAN_SIGNED_VALUES:
            out.append(f"{f['label']}: {f['values']} values, too few for the mean signed difference")
        if abs(f['mean_signed']) > MEAN_SIGNED_BOUND:
            out.append(f"{f['label']}: mean signed difference {f['mean_signed']:+.5f} LSB, bound {MEAN_SIGNED_BOUND:.5f}")
    return out


def resize_findings(fmt, got, planes, rect, out_w, out_h, eps=None, allow=None):
    vd, agree = judge_resize(fmt, got, planes, rect, out_w, out_h, eps, allow)
    return dict(worst=vd.worst, share=vd.share, mean_signed=vd.mean_signed, values=vd.values, agree=agree)


def mean_signed_applies(fmt, rect, out_w, out_h, values, smooth):
    """uint16, smooth frames, enough values, a real resampling in both axes -- and not the exact-2x case: there the area branch rounds the
    quarter-sums half up and the float path half to even, a mean difference of 1/8 LSB between two readings that no float64 sampler can
    choose between."""
    cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
    return fmt == 'u16c3' and smooth and values >= MEAN_SIGNED_VALUES and (cw, ch) != (2 * out_w, 2 * out_h) and (cw, ch) != (out_w, out_h)


def resize_violations(fmt, f, rect, out_w, out_h, smooth):
    out = []
    if f['agree'] > 1e-9 * (TOP[fmt] + 1):
        out.append(f"interpolate and grid_sample disagree at the centre by {f['agree']:.3g}")
    if f['worst'] > 0:
        out.append(f"{f['worst']:.3f} LSB outside the envelope")
    if f['share'] < SHARE_GLOBAL:
        out.append(f"only {f['share']:.3f} of the pixels judged")
    if mean_signed_applies(fmt, rect, out_w, out_h, f['values'], smooth) and abs(f['mean_signed']) > MEAN_SIGNED_BOUND:
        out.append(f"mean signed difference {f['mean_signed']:+.5f} LSB, bound {MEAN_SIGNED_BOUND:.5f}")
    return out


# ---- 4:2:0: the chroma planes ---------------------------------------------------------------------------------------------------------
# Nothing below takes a position, a clamp range or a parity rule from a model: a chroma sample (cx, cy) is said to sit on luma pixel
# (2 cx, 2 cy) -- the definition under test -- and everything else follows from the float64 luma positions above, halved.

def planes_420(fmt, kind, n, H, W, seed=0, device='cpu'):
    """(y (n, H, W, 1), uv (n, H/2, W/2, 2)) float64 planes, kind 'smooth' or 'noise'; the chroma planes have their own phases and draws."""
    make = {'smooth': smooth_planes, 'noise': noise_planes}[kind]
    return make(LUMA_OF[fmt], n, H, W, seed, device), make(CHROMA_OF[fmt], n, H // 2, W // 2, seed + 17, device)


def chroma_ring(u, v, H, W):
    """Chroma samples a sampler of the chroma plane cannot judge, from the luma source (u, v) of their siting pixel: that source lies
    outside [0, W-1] x [0, H-1] -- no cell owns the pixel for certain, so the sample may be the border outright -- while the halved
    position still lies within a chroma pixel of the plane, (-1, Wc) x (-1, Hc), where the sampler blends the plane with the border.  The
    blend zone is one CHROMA pixel wide, two luma pixels: the luma ring is not this ring."""
    outside = (u < 0) | (u > W - 1) | (v < 0) | (v > H - 1)
    return outside & (u / 2 > -1) & (u / 2 < W // 2) & (v / 2 > -1) & (v / 2 < H // 2)


def chroma_far_outside(uc, vc, Hc, Wc):
    """Chroma samples whose source lies well outside the chroma plane: the (U, V) border exactly."""
    return (uc < -1.5) | (uc > Wc + 0.5) | (vc < -1.5) | (vc > Hc + 0.5)


def chroma_setup(setup, H, W):
    """The chroma plane's setup from the luma frame's: the source of the even luma pixels, halved; judged where luma is judged, less the
    chroma ring.  Exact only where every halved position is an integer (identity, shifts even in both axes): an odd shift moves chroma by
    half a chroma pixel, which is judged by the envelope like any other motion."""
    ul, vl = setup.u[:, ::2, ::2], setup.v[:, ::2, ::2]
    uc, vc = ul / 2, vl / 2
    exact = bool(setup.exact and ((uc == uc.round()) & (vc == vc.round())).all())
    judged = ~chroma_ring(ul, vl, H, W) if setup.judged is None else setup.judged[:, ::2, ::2] & ~chroma_ring(ul, vl, H, W)
    return WarpSetup(setup.label, setup.unstab, setup.stab, uc, vc, None if exact else judged, exact,
                     1.0 if exact else min(setup.min_share, SHARE_GLOBAL), chroma_far_outside(uc, vc, H // 2, W // 2))


def chroma_axis(lo, hi, out_len, device='cpu'):
    """One axis of the chroma crop-resize, float64: the position in the chroma plane of each of the out_len / 2 output chroma samples and
    the clamp range (c0, c1).  Output chroma sample c sits on output luma pixel 2 c, whose source in the frame is lo + (2 c + 0.5) cw / out
    - 0.5; halved, that is its place among the chroma samples.  c0 .. c1 are the chroma samples whose own luma pixel (even) lies in
    lo .. hi; a one-pixel crop on an odd pixel has none and takes the sample that covers it."""
    cw = hi - lo + 1
    c0, c1 = -(-lo // 2), hi // 2
    if c0 > c1:
        c0 = c1 = lo // 2
    c = torch.arange(out_len // 2, dtype=torch.float64, device=device)
    return ((lo + ((2 * c + 0.5) * (cw / out_len) - 0.5)) / 2).clamp(c0, c1), (c0, c1)


def judge_resize_chroma(fmt, got, uv, rect, out_w, out_h, eps=None, allow=None):
    """The chroma crop-resize's verdict: the WHOLE chroma plane sampled at the clamped absolute positions; the envelope is resize_eps (in
    ulps of the chroma plane's extent: the positions are absolute) around them, clamped to the same range.  A clamped position is all
    there is to either clamp: two taps clipped to one row give that row whatever the fraction."""
    left, top, right, bottom = rect
    n, Hc, Wc = uv.shape[:3]
    px, limx = chroma_axis(left, right, out_w, uv.device)
    py, limy = chroma_axis(top, bottom, out_h, uv.device)
    u = px[None, None, :].expand(n, out_h // 2, out_w // 2)
    v = py[None, :, None].expand(n, out_h // 2, out_w // 2)
    centre = sample(uv, u, v, None, clamp=True)
    lo, hi = envelope(uv, u, v, resize_eps(fmt, Hc, Wc, eps), None, clamp=True, lim=(limx, limy))
    lo, hi = torch.minimum(lo, centre), torch.maximum(hi, centre)
    return judge(got, centre, lo, hi, VALUE_ALLOW[fmt] if allow is None else allow)


def resize_chroma_findings(fmt, got, uv, rect, out_w, out_h, eps=None, allow=None):
    vd = judge_resize_chroma(fmt, got, uv, rect, out_w, out_h, eps, allow)
    return dict(worst=vd.worst, share=vd.share, mean_signed=vd.mean_signed, values=vd.values, agree=0.0)


def warp_findings_420(fmt, got_y, got_uv, y, uv, setup, border_yuv, smooth=False):
    """A warped pair judged whole: (luma findings, chroma findings, violations of either)."""
    H, W = y.shape[1:3]
    cs = chroma_setup(setup, H, W)
    fy = warp_findings(LUMA_OF[fmt], got_y, y, setup, border_yuv[:1])
    fc = warp_findings(CHROMA_OF[fmt], got_uv, uv, cs, border_yuv[1:])
    return fy, fc, ['luma ' + s for s in warp_violations(LUMA_OF[fmt], fy, setup, smooth)] + \
        ['chroma ' + s for s in warp_violations(CHROMA_OF[fmt], fc, cs, smooth)]


def resize_findings_420(fmt, got_y, got_uv, y, uv, rect, out_w, out_h):
    fy = resize_findings(LUMA_OF[fmt], got_y, y, rect, out_w, out_h)
    fc = resize_chroma_findings(CHROMA_OF[fmt], got_uv, uv, rect, out_w, out_h)
    return fy, fc, ['luma ' + s for s in resize_violations(LUMA_OF[fmt], fy, rect, out_w, out_h, False)] + \
        ['chroma ' + s for s in resize_violations(CHROMA_OF[fmt], fc, rect, out_w, out_h, False)]


# ---- 4:2:0: registration of chroma on luma, without a model of siting -----------------------------------------------------------------
# A linear ramp with integer slopes, y = a + sx x + sy y, and uv[cy, cx, k] = ramp(2 cx, 2 cy) + offset[k].  Bilinear sampling of a linear
# function returns the function, so whatever the motion out_uv[cy, cx, k] - offset[k] and out_y[2 cy, 2 cx] are the same number ramp(u, v),
# each read through its own coordinate error and its own rounding.  Chroma sited anywhere else is off by its distance times the slope.

RAMP = {'nv12': dict(a=5, sx=3, sy=1, offsets=(0, 7)), 'p010': dict(a=200, sx=100, sy=60, offsets=(0, 500))}
# the warp case of each format: 8 bits need a frame narrow enough for a slope of 3 (5 + 3 * 63 + 47 + 7 = 248): a luma pixel is 4 LSB
REGISTRATION_WARP = {'nv12': WarpCase('homography', 2, 48, 64, 4, 6, 2), 'p010': WarpCase('homography', 2, 270, 484, 5, 7, 2)}
# (n, H, W, rect, size): odd left and top, a non-integer ratio, inside the ramp's range
REGISTRATION_RESIZE = {'nv12': (1, 48, 64, (5, 3, 58, 44), (40, 30)), 'p010': (1, 270, 484, (41, 31, 443, 238), (300, 170))}


def ramp_420(fmt, n, H, W, device='cpu'):
    r = RAMP[fmt]
    xs, ys = pixels(n, H, W, device)
    y = (r['a'] + r['sx'] * xs + r['sy'] * ys)[..., None]
    uv = torch.cat([y[:, ::2, ::2] + o for o in r['offsets']], dim=-1)
    assert float(uv.max()) <= TOP[LUMA_OF[fmt]]
    return y, uv


def _registration_gap(fmt, got_y, got_uv, inside):
    off = torch.tensor(RAMP[fmt]['offsets'], dtype=torch.float64, device=got_y.device)
    gap = ((got_uv - off) - got_y[:, ::2, ::2]).abs() * inside[..., None]
    return float(gap.max()), int(inside.sum())


def registration_warp(fmt, got_y, got_uv, setup):
    """(worst |chroma - luma at the even pixel| in LSB, samples compared, bound) of a warped ramp.  Compared where every tap of both
    lies inside the frame (the luma source within [1, W - 3] x [1, H - 3]): against the border nothing is linear.
    Bound: the luma bucket moves the source by up to 1/64 luma px per axis, the chroma bucket by 1/64 chroma px = 1/32 luma px; each side
    then rounds once (0.5 LSB), in float32 for 16 bits (VALUE_ALLOW), with 2^15 fixed-point weights for 8 bits (four taps, each weight
    within 2^-16 of its value, on taps that differ by at most sx + sy: below 0.001 LSB)."""
    H, W = got_y.shape[1:3]
    u, v = setup.u[:, ::2, ::2], setup.v[:, ::2, ::2]
    inside = (u >= 1) & (u <= W - 3) & (v >= 1) & (v <= H - 3)
    if setup.judged is not None:
        inside = inside & setup.judged[:, ::2, ::2]
    r = RAMP[fmt]
    value = VALUE_ALLOW[CHROMA_OF[fmt]] if fmt == 'p010' else 0.5 + 0.001
    eps = warp_eps(LUMA_OF[fmt], H, W) + 2 * warp_eps(CHROMA_OF[fmt], H // 2, W // 2)
    return (*_registration_gap(fmt, got_y, got_uv, inside), (r['sx'] + r['sy']) * (1 / 64 + 1 / 32 + eps) + 2 * value)


def registration_resize(fmt, got_y, got_uv, H, W, rect, out_w, out_h):
    """The same for a crop-resize, on the samples that neither the luma rule (the position clamped to the crop) nor the chroma rule (clamped
    to c0 .. c1) clamps, decided here from the float64 positions.  Bound: no bucket, the float32 position alone (resize_eps, at most
    RESIZE_EPS_CAP) times the slope, and each side's value error: 16 bits VALUE_ALLOW; 8 bits between -(0.5 + 0.25 + 0.25 + 1/32) and
    +0.5 of the float64 value (the final rounding; two products truncated to quarter LSBs; the >> 4 of both rows and the 11-bit weights
    on taps 3 LSB apart) -- the same one-sided range on both sides, so their difference stays below its width."""
    left, top, right, bottom = rect
    r = RAMP[fmt]
    keep = []
    for lo, hi, out_len in ((left, right, out_w), (top, bottom, out_h)):
        c = torch.arange(out_len // 2, dtype=torch.float64, device=got_y.device)
        p = lo + (2 * c + 0.5) * ((hi - lo + 1) / out_len) - 0.5                     # luma source of output luma pixel 2 c, absolute
        pc, (c0, c1) = chroma_axis(lo, hi, out_len, got_y.device)
        keep.append((p >= lo) & (p <= hi) & (p / 2 >= c0) & (p / 2 <= c1) & (pc == p / 2))
    inside = (keep[1][:, None] & keep[0][None, :])[None].expand(got_uv.shape[:3])
    value = 2 * VALUE_ALLOW[CHROMA_OF[fmt]] if fmt == 'p010' else 1.0 + 0.5 + 1 / 32
    return (*_registration_gap(fmt, got_y, got_uv, inside), (r['sx'] + r['sy']) * 3 * RESIZE_EPS_CAP + value)
