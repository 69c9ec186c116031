// csrc/scores_body.h on the host, under the address and undefined-behaviour sanitizers: the scores of one clip written with the header's
// functions in the kernel's formulation (256 strided partials, a halving tree per 64, (w0 + w1) + (w2 + w3)), against cases dumped from
// tests/scores_model.py by tools/scores_dump_cases.py.  Scores, per-pair values and record of every case must equal the model's bit for bit.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/scores_body_check.cpp -o scores_body_check
//   python tools/scores_dump_cases.py cases.bin && ./scores_body_check cases.bin
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../meshflow_amd/csrc/scores_body.h"

using namespace mf::scores;

struct Parts { double sum; float least; bool nan; int count, first; };

static void fold(Parts& v, const Parts& o)
{
    v.sum = v.sum + o.sum;
    v.least = smaller(v.least, o.least);
    v.nan = v.nan || o.nan;
    v.count += o.count;
    v.first = o.first < v.first ? o.first : v.first;
}

// one clip, as feature_scores_kernel does it (info: empty = no record)
static void score(const std::vector<double>& hom, const std::vector<int32_t>& info, int P, float (&out)[2], std::vector<float>& per_pair, int32_t (&record)[2])
{
    std::vector<Parts> part((size_t)LANES, Parts{0.0, __builtin_inff(), false, 0, P});
    for (int lane = 0; lane < LANES; ++lane)
        for (int p = lane; p < P; p += LANES) {
            Parts& v = part.at((size_t)lane);
            float ratio = quiet_nan(), distortion = quiet_nan();
            if (info.empty() || info.at(4 * (size_t)p) == OK) {
                double h[9];
                for (int i = 0; i < 9; ++i) h[i] = hom.at(9 * (size_t)p + i);
                pair_scores(h, ratio, distortion);
                v.sum = v.sum + (double)ratio;
                v.least = smaller(v.least, distortion);
                v.nan = v.nan || distortion != distortion;
                ++v.count;
            } else if (p < v.first) {
                v.first = p;
            }
            per_pair.at(2 * (size_t)p) = ratio;
            per_pair.at(2 * (size_t)p + 1) = distortion;
        }
    for (int w = 0; w < LANES / WAVE; ++w)
        for (int step = WAVE / 2; step > 0; step >>= 1)
            for (int j = 0; j < step; ++j) fold(part.at((size_t)(w * WAVE + j)), part.at((size_t)(w * WAVE + j + step)));
    Parts lo = part.at(0), hi = part.at(2 * (size_t)WAVE);
    fold(lo, part.at((size_t)WAVE));
    fold(hi, part.at(3 * (size_t)WAVE));
    fold(lo, hi);
    clip_scores(lo.sum, lo.count, lo.least, lo.nan, out[0], out[1]);
    record[0] = lo.count; record[1] = lo.first < P ? lo.first : -1;
}

template <class T> static bool read(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int32_t head[2];
    if (!f || !read(f, head, 2) || head[0] != 0x524F4353) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    long pairs = 0, scored = 0, with_record = 0, nan_scores = 0, bad = 0;
    for (int c = 0; c < head[1]; ++c) {
        int32_t shape[2];
        if (!read(f, shape, 2) || shape[0] < 1 || shape[0] > MAX_PAIRS) return 2;
        const int P = shape[0];
        std::vector<double> hom(9 * (size_t)P);
        std::vector<int32_t> info(shape[1] ? 4 * (size_t)P : 0);
        std::vector<float> want_pairs(2 * (size_t)P), per_pair(2 * (size_t)P);
        float want[2], out[2];
        int32_t want_record[2], record[2];
        if (!read(f, hom.data(), hom.size()) || (!info.empty() && !read(f, info.data(), info.size())) || !read(f, want, 2) || !read(f, want_pairs.data(), want_pairs.size()) ||
            !read(f, want_record, 2))
            return 2;
        score(hom, info, P, out, per_pair, record);
        pairs += P; scored += record[0]; with_record += shape[1] ? 1 : 0;
        nan_scores += (out[0] != out[0]) + (out[1] != out[1]);
        const bool s_bad = memcmp(out, want, sizeof out) != 0, r_bad = memcmp(record, want_record, sizeof record) != 0,
                   p_bad = memcmp(per_pair.data(), want_pairs.data(), per_pair.size() * sizeof(float)) != 0;
        if (s_bad || r_bad || p_bad) {
            ++bad;
            printf("case %d (P = %d): scores (%.9g, %.9g), model (%.9g, %.9g); record (%d, %d), model (%d, %d)\n", c, P, out[0], out[1], want[0], want[1],
                   record[0], record[1], want_record[0], want_record[1]);
            for (int p = 0, shown = 0; p < 2 * P && shown < 5; ++p)
                if (memcmp(&per_pair.at((size_t)p), &want_pairs.at((size_t)p), 4)) {
                    printf("    pair %d %s: %.9g, model %.9g\n", p / 2, p % 2 ? "distortion" : "ratio", per_pair.at((size_t)p), want_pairs.at((size_t)p));
                    ++shown;
                }
        }
    }
    fclose(f);
    printf("scores_body_check: %d cases (%ld with a fit record), %ld pairs, %ld scored, %ld NaN scores, %ld mismatches\n", head[1], with_record, pairs,
           scored, nan_scores, bad);
    return bad ? 1 : 0;
}
