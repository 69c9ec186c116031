// csrc/hfit_body.h on the host, under the address and undefined-behaviour sanitizers: the fit of one pair written with the header's
// functions in the kernels' formulation (256 strided partial sums, a halving tree per 64, (w0 + w1) + (w2 + w3); the 9 x 9 matrices in
// plain arrays, column k of a rotation after column k - 1), against cases dumped from tests/homography_model.py by tools/hfit_dump_cases.py.
// H, info and diag of every case must equal the model's bit for bit.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/hfit_body_check.cpp -o hfit_body_check
//   python tools/hfit_dump_cases.py cases.bin && ./hfit_body_check cases.bin
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../meshflow_amd/csrc/hfit_body.h"

using namespace mf::hfit;

// the ordered sums of hfit_sums_kernel: terms(i, t) fills the N terms of point i
template <int N, class Terms> static void ordered_sums(int K, Terms terms, double (&total)[N])
{
    std::vector<double> partial((size_t)LANES * N, 0.0);
    for (int lane = 0; lane < LANES; ++lane)
        for (int i = lane; i < K; i += LANES) {
            double t[N];
            terms(i, t);
            for (int q = 0; q < N; ++q) partial.at((size_t)lane * N + q) = partial.at((size_t)lane * N + q) + t[q];
        }
    double wave[LANES / WAVE][N];
    for (int w = 0; w < LANES / WAVE; ++w) {
        for (int step = WAVE / 2; step > 0; step >>= 1)
            for (int j = 0; j < step; ++j)
                for (int q = 0; q < N; ++q) {
                    double& v = partial.at((size_t)(w * WAVE + j) * N + q);
                    v = v + partial.at((size_t)(w * WAVE + j + step) * N + q);
                }
        for (int q = 0; q < N; ++q) wave[w][q] = partial.at((size_t)(w * WAVE) * N + q);
    }
    for (int q = 0; q < N; ++q) total[q] = (wave[0][q] + wave[1][q]) + (wave[2][q] + wave[3][q]);
}

// one pair, as hfit_sums_kernel and hfit_solve_kernel do it
static void fit(const std::vector<double>& e, const std::vector<double>& l, double (&H)[9], int32_t (&info)[4], double (&diag)[8])
{
    const int K = (int)(e.size() / 2);
    const double kf = (double)K;
    for (int i = 0; i < 9; ++i) H[i] = i % 4 == 0 ? 1.0 : 0.0;
    for (double& d : diag) d = 0.0;
    info[0] = OK; info[1] = K; info[2] = 0; info[3] = 0;
    if (K < 4) { info[0] = TOO_FEW; return; }
    double first[4], c[4], second[MOMENTS], sim[6], third[SUMS];
    ordered_sums<4>(K, [&](int i, double (&t)[4]) { t[0] = e.at(2 * i); t[1] = e.at(2 * i + 1); t[2] = l.at(2 * i); t[3] = l.at(2 * i + 1); }, first);
    for (int q = 0; q < 4; ++q) { c[q] = first[q] / kf; diag[2 + q] = c[q]; }
    ordered_sums<MOMENTS>(K, [&](int i, double (&t)[MOMENTS]) { moment_terms(e.at(2 * i), e.at(2 * i + 1), l.at(2 * i), l.at(2 * i + 1), c, t); }, second);
    if (collinear(second[1], second[2], second[3]) || collinear(second[5], second[6], second[7])) { info[0] = COLLINEAR; return; }
    similarity(second[0], second[4], kf, c, sim);
    diag[0] = sim[0]; diag[1] = sim[1];
    ordered_sums<SUMS>(K, [&](int i, double (&t)[SUMS]) { normal_terms(e.at(2 * i), e.at(2 * i + 1), l.at(2 * i), l.at(2 * i + 1), sim, t); }, third);
    double work[24] = {};
    memcpy(work, third, sizeof third);
    double A[81], V[81];
    for (int at = 0; at < 81; ++at) { A[at] = normal_entry(work, kf, at / 9, at % 9); V[at] = at / 9 == at % 9 ? 1.0 : 0.0; }
    int sweeps = 0;
    bool converged = false;
    for (int sweep = 1; sweep <= MAX_SWEEPS && !converged; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double app = A[p * 9 + p], aqq = A[q * 9 + q], apq = A[p * 9 + q];
                double t, cs, sn;
                if (!rotation(app, aqq, apq, t, cs, sn)) continue;
                rotated = true;
                for (int k = 0; k < 9; ++k) rotate_column(A, V, k, p, q, app, aqq, apq, t, cs, sn);
            }
        sweeps = sweep;
        converged = !rotated;
    }
    const int index = smallest(A, diag[6], diag[7]);
    info[2] = sweeps; info[3] = index;
    if (!converged) { info[0] = NOT_CONVERGED; return; }
    double sim2[6] = {diag[0], diag[1]}, c2[4] = {diag[2], diag[3], diag[4], diag[5]};
    translations(c2, sim2);
    if (!denormalise(V, index, sim2, c2, H)) info[0] = AT_INFINITY;
}

template <class T> static bool read(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int32_t head[2];
    if (!f || !read(f, head, 2) || head[0] != 0x54494648) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    long points = 0, sweeps = 0, by_status[5] = {0, 0, 0, 0, 0}, bad = 0;
    int most = 0;
    for (int c = 0; c < head[1]; ++c) {
        int32_t K;
        if (!read(f, &K, 1) || K < 0) return 2;
        std::vector<double> e(2 * (size_t)K), l(2 * (size_t)K);
        double want_h[9], want_diag[8], H[9], diag[8];
        int32_t want_info[4], info[4];
        if (!read(f, e.data(), e.size()) || !read(f, l.data(), l.size()) || !read(f, want_h, 9) || !read(f, want_info, 4) || !read(f, want_diag, 8)) return 2;
        fit(e, l, H, info, diag);
        points += K; sweeps += info[2];
        most = info[2] > most ? info[2] : most;
        if (info[0] >= 0 && info[0] < 5) ++by_status[info[0]];
        const bool h_bad = memcmp(H, want_h, sizeof H) != 0, i_bad = memcmp(info, want_info, sizeof info) != 0, d_bad = memcmp(diag, want_diag, sizeof diag) != 0;
        if (h_bad || i_bad || d_bad) {
            ++bad;
            printf("case %d (K = %d): got info (%d, %d, %d, %d), model (%d, %d, %d, %d)%s%s\n", c, K, info[0], info[1], info[2], info[3], want_info[0],
                   want_info[1], want_info[2], want_info[3], h_bad ? ", H differs" : "", d_bad ? ", diag differs" : "");
            for (int i = 0; i < 8; ++i)
                if (memcmp(&diag[i], &want_diag[i], 8)) printf("    diag[%d]: %.17g, model %.17g\n", i, diag[i], want_diag[i]);
        }
    }
    fclose(f);
    printf("hfit_body_check: %d cases (%ld ok, %ld too few, %ld collinear, %ld at infinity, %ld not converged), %ld points, %ld sweeps (at most %d), "
           "%ld mismatches\n", head[1], by_status[0], by_status[1], by_status[2], by_status[3], by_status[4], points, sweeps, most, bad);
    return bad ? 1 : 0;
}
