// csrc/track_body.h on the host, under the address and undefined-behaviour sanitizers: FAST, the pyramid and pyramidal LK of whole images,
// written with the header's functions in the kernels' formulation (LDS tile -> arrays), against cases dumped from tests/track_model.py by
// tools/track_dump_cases.py.  Every corner, position and flag must equal the model's bit for bit.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/track_body_check.cpp -o track_body_check
//   python tools/track_dump_cases.py cases.bin && ./track_body_check cases.bin
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../meshflow_amd/csrc/track_body.h"

using namespace mf::track;

struct Image { int w, h; std::vector<uint8_t> px; uint8_t at(int x, int y) const { return px.at((size_t)y * w + x); } };

static std::vector<float> fast(const Image& im, int threshold)
{
    static const int DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    static const int DY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    std::vector<int> score((size_t)im.w * im.h, 0);
    for (int y = 3; y < im.h - 3; ++y)
        for (int x = 3; x < im.w - 3; ++x) {
            int d[16];
            for (int i = 0; i < 16; ++i) d[i] = (int)im.at(x, y) - (int)im.at(x + DX[i], y + DY[i]);
            const int best = fast_best(d);
            score[(size_t)y * im.w + x] = best > threshold ? best - 1 : 0;
        }
    std::vector<float> out;
    for (int y = 0; y < im.h; ++y)
        for (int x = 0; x < im.w; ++x) {
            const int mine = score[(size_t)y * im.w + x];
            bool keep = mine > 0;
            for (int j = -1; j <= 1 && keep; ++j)
                for (int i = -1; i <= 1; ++i) {
                    if ((i == 0 && j == 0) || x + i < 0 || x + i >= im.w || y + j < 0 || y + j >= im.h) continue;
                    keep = keep && mine > score[(size_t)(y + j) * im.w + x + i];
                }
            if (keep) { out.push_back((float)x); out.push_back((float)y); }
        }
    return out;
}

static Image pyr_down(const Image& s)
{
    Image d;
    d.w = (s.w + 1) / 2; d.h = (s.h + 1) / 2;
    d.px.resize((size_t)d.w * d.h);
    std::vector<int> sums((size_t)s.h * d.w);
    for (int y = 0; y < s.h; ++y)
        for (int ox = 0; ox < d.w; ++ox)
            sums[(size_t)y * d.w + ox] = pyr_taps(s.at(reflect101(2 * ox - 2, s.w), y), s.at(reflect101(2 * ox - 1, s.w), y), s.at(2 * ox, y),
                                                  s.at(reflect101(2 * ox + 1, s.w), y), s.at(reflect101(2 * ox + 2, s.w), y));
    for (int oy = 0; oy < d.h; ++oy)
        for (int ox = 0; ox < d.w; ++ox) {
            int r[5];
            for (int k = 0; k < 5; ++k) r[k] = sums[(size_t)reflect101(2 * oy - 2 + k, s.h) * d.w + ox];
            d.px[(size_t)oy * d.w + ox] = (uint8_t)((pyr_taps(r[0], r[1], r[2], r[3], r[4]) + 128) >> 8);
        }
    return d;
}

// one level of one feature, as lk_level_kernel does it
static void lk_level(const Image& I, const Image& J, int level, int top, float ptx, float pty, float& nx, float& ny, int& ok)
{
    const float scale = 1.f / (float)(1 << level);
    const float px = ptx * scale, py = pty * scale;
    if (level == top) { nx = px; ny = py; ok = 1; } else { nx = nx * 2.f; ny = ny * 2.f; }
    const float hx = px - 10.f, hy = py - 10.f;
    const int ix = floor_sat(hx), iy = floor_sat(hy);
    bool tracking = !outside(ix, iy, I.w, I.h);
    Matrix m = {0.f, 0.f, 0.f, 0.f};
    int Iv[POSITIONS], Ixv[POSITIONS], Iyv[POSITIONS];
    if (tracking) {
        uint8_t tile[TILE][TILE];
        int16_t dxs[GRID][GRID], dys[GRID][GRID];
        for (int r = 0; r < TILE; ++r)
            for (int c = 0; c < TILE; ++c) tile[r][c] = I.at(reflect101(ix - 1 + c, I.w), reflect101(iy - 1 + r, I.h));
        for (int r = 0; r < GRID; ++r)
            for (int c = 0; c < GRID; ++c) {
                int dx = 0, dy = 0;
                if (ix + c >= 0 && ix + c < I.w && iy + r >= 0 && iy + r < I.h) {
                    int t0[3], t1[3];
                    for (int q = 0; q < 3; ++q) {
                        const int a = tile[r][c + q], b = tile[r + 1][c + q], e = tile[r + 2][c + q];
                        t0[q] = (a + e) * 3 + b * 10;
                        t1[q] = e - a;
                    }
                    dx = t0[2] - t0[0];
                    dy = (t1[0] + t1[2]) * 3 + t1[1] * 10;
                }
                dxs[r][c] = (int16_t)dx; dys[r][c] = (int16_t)dy;
            }
        const Weights w = lk_weights(hx - (float)ix, hy - (float)iy);
        long long s11 = 0, s12 = 0, s22 = 0;
        for (int q = 0; q < POSITIONS; ++q) {
            const int r = q / WIN, c = q % WIN;
            Iv[q] = blend(w, tile[r + 1][c + 1], tile[r + 1][c + 2], tile[r + 2][c + 1], tile[r + 2][c + 2], W_BITS - 5);
            Ixv[q] = blend(w, dxs[r][c], dxs[r][c + 1], dxs[r + 1][c], dxs[r + 1][c + 1], W_BITS);
            Iyv[q] = blend(w, dys[r][c], dys[r][c + 1], dys[r + 1][c], dys[r + 1][c + 1], W_BITS);
            s11 += (long long)Ixv[q] * Ixv[q]; s12 += (long long)Ixv[q] * Iyv[q]; s22 += (long long)Iyv[q] * Iyv[q];
        }
        tracking = lk_matrix(s11, s12, s22, m);
    }
    if (!tracking) {
        if (level == 0) ok = 0;
    } else {
        float fx = nx - 10.f, fy = ny - 10.f, pdx = 0.f, pdy = 0.f;
        for (int it = 0; it < MAX_COUNT; ++it) {
            const int jx = floor_sat(fx), jy = floor_sat(fy);
            if (outside(jx, jy, J.w, J.h)) {
                if (level == 0) ok = 0;
                break;
            }
            const Weights w = lk_weights(fx - (float)jx, fy - (float)jy);
            long long sb1 = 0, sb2 = 0;
            for (int q = 0; q < POSITIONS; ++q) {
                const int r = q / WIN, c = q % WIN;
                const int y0 = reflect101(jy + r, J.h), y1 = reflect101(jy + r + 1, J.h), x0 = reflect101(jx + c, J.w), x1 = reflect101(jx + c + 1, J.w);
                const int diff = blend(w, J.at(x0, y0), J.at(x1, y0), J.at(x0, y1), J.at(x1, y1), W_BITS - 5) - Iv[q];
                sb1 += (long long)diff * Ixv[q]; sb2 += (long long)diff * Iyv[q];
            }
            float dx, dy;
            lk_delta(m, sb1, sb2, dx, dy);
            fx = fx + dx; fy = fy + dy;
            nx = fx + 10.f; ny = fy + 10.f;
            const int leave = lk_exit(dx, dy, pdx, pdy, it);
            if (leave == 2) { nx = nx - dx * 0.5f; ny = ny - dy * 0.5f; }
            if (leave) break;
            pdx = dx; pdy = dy;
        }
    }
    if (level == 0 && ok && outside(floor_sat(nx - 10.f), floor_sat(ny - 10.f), I.w, I.h)) ok = 0;
}

template <class T> static bool read(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int32_t head[2];
    if (!f || !read(f, head, 2) || head[0] != 0x4b545246) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    long corners = 0, tracks = 0, levels = 0, bad = 0;
    for (int c = 0; c < head[1]; ++c) {
        int32_t dims[4];                                        // w, h, points, corners
        if (!read(f, dims, 4)) return 2;
        Image e{dims[0], dims[1], std::vector<uint8_t>((size_t)dims[0] * dims[1])}, l = e;
        std::vector<float> pts(2 * (size_t)dims[2]), want_moved(pts.size()), want_corners(2 * (size_t)dims[3]);
        std::vector<uint8_t> want_found(dims[2]);
        if (!read(f, e.px.data(), e.px.size()) || !read(f, l.px.data(), l.px.size()) || !read(f, pts.data(), pts.size()) ||
            !read(f, want_corners.data(), want_corners.size()) || !read(f, want_moved.data(), want_moved.size()) ||
            !read(f, want_found.data(), want_found.size())) return 2;
        const std::vector<float> got = fast(e, 10);
        corners += (long)got.size() / 2;
        if (got.size() != want_corners.size() || (got.size() && memcmp(got.data(), want_corners.data(), got.size() * 4))) { ++bad; printf("case %d: corners differ\n", c); }
        const int top = top_level(e.w, e.h);
        std::vector<Image> pe{e}, pl{l};
        for (int k = 1; k <= top; ++k) { pe.push_back(pyr_down(pe.back())); pl.push_back(pyr_down(pl.back())); }
        for (int k = 0; k <= top; ++k) {
            int lw, lh;
            level_size(e.w, e.h, k, lw, lh);
            if (lw != pe[k].w || lh != pe[k].h) { ++bad; printf("case %d: level %d size\n", c, k); }
        }
        levels += top + 1;
        for (int p = 0; p < dims[2]; ++p) {
            float nx = 0.f, ny = 0.f;
            int ok = 1;
            for (int level = top; level >= 0; --level) lk_level(pe[level], pl[level], level, top, pts[2 * p], pts[2 * p + 1], nx, ny, ok);
            ++tracks;
            if (memcmp(&nx, &want_moved[2 * p], 4) || memcmp(&ny, &want_moved[2 * p + 1], 4) || ok != want_found[p]) {
                ++bad;
                printf("case %d point %d: got (%.9g, %.9g) %d, model (%.9g, %.9g) %d\n", c, p, nx, ny, ok, want_moved[2 * p], want_moved[2 * p + 1], want_found[p]);
            }
        }
    }
    fclose(f);
    printf("track_body_check: %d cases, %ld corners, %ld pyramid levels, %ld tracks, %ld mismatches\n", head[1], corners, levels, tracks, bad);
    return bad ? 1 : 0;
}
