// main.cpp -- mfx_train, the command-line driver over libmfx.
//
// Speaks the reference driver's protocol (reference: src/main.cpp:38-173): the same flags, the same
// log lines in the same order, the same post-run checks -- so that scripts written against the
// reference (scripts/times.sh and friends) keep working -- with the GPU leg served by this repository's
// HIP implementation behind kernel_wrapper_{ccdpp,als}_NV.  Two steps the reference only stubs out are
// real here: -save <file> (model dump) and -predict (file-based scoring); -recommend adds top-N lists and their
// ranking metrics.  The reference's -OMP leg is
// its CPU solver, which is not part of the product (the CPU restatement lives under oracle/ as a test
// oracle): here -OMP runs the library's REFERENCE-ORDER parity modes on the GPU -- for CCD++ the sweeps that
// add every column strictly left to right in fp32 (csrc/ccd_reforder.hip), for ALS the reference's own
// operation order (csrc/als_exact.hip); both reproduce src/CCD.cpp / src/ALS.cpp bit for bit -- from the same
// initial factors, so that the driver's closing golden_compare checks the fast path against the reference's
// arithmetic exactly as the reference's -CUDA -OMP run checks its GPU path against its CPU path.  The leg says
// what it is in the log and does NOT print its time under the OMP name: a script that divides "OMP Training
// time" by "CUDA Training time" must not mistake a GPU/GPU ratio for a CPU speed-up.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "reference_api.hpp"
#include "tools.hpp"

namespace {

struct Stopwatch {
    std::chrono::high_resolution_clock::time_point origin = std::chrono::high_resolution_clock::now();
    double seconds() const { return std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - origin).count(); }
};

void rule() { puts("------------------------------------------------------------"); }

// Factor pair in the solver's layout: CCD++ keeps k rows of length rows/cols, ALS rows/cols rows of
// length k; both start from the reference's initial_col stream.
struct Factors {
    MatData W, H;
    Factors(bool als, unsigned k, long rows, long cols) {
        if (als) { initial_col(W, rows, k); initial_col(H, cols, k); }
        else { initial_col(W, k, rows); initial_col(H, k, cols); }
    }
};

void solve_on_gpu(SparseMatrix& R, TestData& T, Factors& f, parameter& prm, bool als) {
    if (als) kernel_wrapper_als_NV(R, T, f.W, f.H, prm);
    else if (prm.n_gpus > 1) kernel_wrapper_ccdpp_multi(R, T, f.W, f.H, prm, prm.n_gpus);
    else kernel_wrapper_ccdpp_NV(R, T, f.W, f.H, prm);
}

// -predict <model> <test.txt> <output>: file-based scoring; the model must be row-major (rows x k),
// i.e. written by an ALS run with -save, or converted.
int predict_from_files(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: mfx_train -predict model_file test_file output_file\n"); return EXIT_FAILURE; }
    const char* names[3] = {argv[2], argv[3], argv[4]};
    const char* modes[3] = {"rb", "r", "w"};
    const char* what[3] = {"model", "test", "output"};
    FILE* fp[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; ++i) {
        fp[i] = fopen(names[i], modes[i]);
        if (!fp[i]) {
            fprintf(stderr, "can't open %s file %s\n", what[i], names[i]);
            for (int j = 0; j < i; ++j) fclose(fp[j]);
            return EXIT_FAILURE;
        }
    }
    calculate_rmse_from_file(fp[0], fp[1], fp[2]);
    for (FILE* f : fp) fclose(f);
    return EXIT_SUCCESS;
}

// -recommend <model> <data_dir> <N> <output> [min_rating]: top-N lists for every user of a -save model (W rows x k,
// then H cols x k, row-major), excluding each user's training ratings; one line "u i_1 ... i_N" per user (1-based,
// unfilled slots omitted), then the ranking metrics of the lists against the test set of data_dir.
int recommend_from_files(int argc, char** argv) {
    if (argc != 6 && argc != 7) {
        fprintf(stderr, "usage: mfx_train -recommend model_file data_dir N output_file [min_rating]\n");
        return EXIT_FAILURE;
    }
    char* end = nullptr;
    const long n_top = strtol(argv[4], &end, 10);
    if (!end || *end || n_top < 1 || n_top > 1024) {
        fprintf(stderr, "-recommend: N must be an integer in [1, 1024] (got %s)\n", argv[4]);
        return EXIT_FAILURE;
    }
    float min_rating = -INFINITY;
    if (argc == 7) {
        min_rating = strtof(argv[6], &end);
        if (!end || *end || std::isnan(min_rating)) {
            fprintf(stderr, "-recommend: bad min_rating %s\n", argv[6]);
            return EXIT_FAILURE;
        }
    }
    FILE* fm = fopen(argv[2], "rb");
    if (!fm) { fprintf(stderr, "can't open model file %s\n", argv[2]); return EXIT_FAILURE; }
    long hdr[2][2] = {{0, 0}, {0, 0}};
    std::vector<float> W, H;
    bool ok = fread(hdr[0], sizeof(long), 2, fm) == 2 && hdr[0][0] > 0 && hdr[0][1] > 0;
    if (ok) {
        W.resize((size_t) hdr[0][0] * hdr[0][1]);
        ok = fread(W.data(), sizeof(float), W.size(), fm) == W.size();
    }
    ok = ok && fread(hdr[1], sizeof(long), 2, fm) == 2 && hdr[1][0] > 0 && hdr[1][1] > 0;
    if (ok) {
        H.resize((size_t) hdr[1][0] * hdr[1][1]);
        ok = fread(H.data(), sizeof(float), H.size(), fm) == H.size();
    }
    fclose(fm);
    if (!ok || hdr[0][1] != hdr[1][1]) {
        fprintf(stderr, "model file %s: expected W (rows x k) then H (cols x k) as written by -save\n", argv[2]);
        return EXIT_FAILURE;
    }
    const long k = hdr[0][1];

    SparseMatrix R;
    TestData T;
    load(argv[3], R, T);
    if (R.rows != hdr[0][0] || R.cols != hdr[1][0]) {
        fprintf(stderr, "model is %ld x %ld (k = %ld) but %s holds a %ld x %ld rating matrix\n", hdr[0][0], hdr[1][0], k,
                argv[3], R.rows, R.cols);
        return EXIT_FAILURE;
    }
    const Stopwatch sw;
    mfx_csx ex{};
    ex.rows = R.rows;
    ex.cols = R.cols;
    ex.nnz = R.nnz;
    ex.csr_row_ptr = R.get_csr_row_ptr();
    ex.csr_col_idx = R.get_csr_col_indx();
    mfx_rec_t rec = nullptr;
    std::vector<uint32_t> items((size_t) R.rows * n_top);
    int rc = mfx_rec_create(&rec, W.data(), H.data(), R.rows, R.cols, k, 1, &ex, MFX_HOST, 0);
    if (rc == MFX_OK) rc = mfx_rec_query(rec, R.rows, nullptr, (int32_t) n_top, items.data(), nullptr, MFX_HOST, 0);
    mfx_rec_destroy(rec);
    if (rc != MFX_OK) { fprintf(stderr, "RECOMMEND FAILED: %s\n", mfx_last_error()); return EXIT_FAILURE; }
    printf("[info] Top-%ld recommendation for %ld users: %lf s.\n", n_top, R.rows, sw.seconds());

    FILE* fo = fopen(argv[5], "w");
    if (!fo) { fprintf(stderr, "can't open output file %s\n", argv[5]); return EXIT_FAILURE; }
    for (long u = 0; u < R.rows; ++u) {
        fprintf(fo, "%ld", u + 1);
        for (long j = 0; j < n_top; ++j) {
            const uint32_t it = items[(size_t) u * n_top + j];
            if (it != 0xFFFFFFFFu) fprintf(fo, " %u", it + 1);
        }
        fputc('\n', fo);
    }
    fclose(fo);

    const Stopwatch sm;
    mfx_coo coo{T.nnz, T.getTestRow(), T.getTestCol(), T.getTestVal()};
    double m[4] = {0, 0, 0, 0};
    int64_t evaluated = 0;
    rc = mfx_topn_metrics(R.rows, nullptr, (int32_t) n_top, items.data(), &coo, min_rating, m, &evaluated);
    if (rc != MFX_OK) { fprintf(stderr, "metrics failed: %s\n", mfx_last_error()); return EXIT_FAILURE; }
    printf("[FINAL INFO] Top-N (N = %ld) over %lld users: HR = %.8f Precision = %.8f Recall = %.8f NDCG = %.8f "
           "Calculated in %lfs\n", n_top, (long long) evaluated, m[0], m[1], m[2], m[3], sm.seconds());
    return EXIT_SUCCESS;
}

const char* option_value(int argc, char** argv, const char* flag) {
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], flag)) return argv[i + 1];
    return nullptr;
}

}  // namespace

int main(int argc, char* argv[]) {
    if (argc > 1 && !strcmp(argv[1], "-predict")) return predict_from_files(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "-recommend")) return recommend_from_files(argc, argv);
    const Stopwatch whole_run;
    parameter prm = parse_command_line(argc, argv);
    const char* model_path = option_value(argc, argv, "-save");

    SparseMatrix R;
    TestData T;
    rule();
    puts("[info] Loading R matrix...");
    {
        const Stopwatch sw;
        load(prm.src_dir, R, T);
        printf("[info] Loading rating data time: %lf s.\n", sw.seconds());
    }
    rule();

    const bool als = prm.solver_type == solvertype::ALS;
    puts(als ? "[info] Picked Version: ALS!" : "[info] Picked Version: CCD!");
    Factors solved(als, prm.k, R.rows, R.cols), untouched(als, prm.k, R.rows, R.cols);
    printf("[info] ThreadsPerBlock = %u | Blocks = %u | K = %u | InnerIter = %d | OuterIter = %d | Threads = %d | L = %.3f\n",
           prm.nThreadsPerBlock, prm.nBlocks, prm.k, prm.maxinneriter, prm.maxiter, prm.threads, prm.lambda);

    if (prm.enable_cuda) {
        rule();
        puts("[INFO] Computing with CUDA...");
        const Stopwatch sw;
        solve_on_gpu(R, T, solved, prm, als);
        printf("[info] CUDA Training time: %lf s.\n", sw.seconds());
        rule();
        calculate_rmse_directly(solved.W, solved.H, T, prm.k, als);
    }
    if (prm.enable_omp) {
        rule();
        puts("[INFO] -OMP: this build has no CPU solver; computing the reference-order leg on the GPU "
             "(same arithmetic and summation order as the reference's CPU solver, bit-identical factors)...");
        parameter second = prm;
        second.schedule = 0;         // ALS: als_exact.hip; CCD++: one launch per reference kernel ...
        second.kernel_variant = -1;  // ... with the sweeps in the reference's summation order (ccd_reforder.hip)
        second.n_gpus = 1;           // a sharded sum has no reference order
        if (second.libpmf_flags) {   // -e / -N change the arithmetic: the reference ignores them, and so does its stand-in leg
            puts("[INFO] -OMP: the reference ignores -e / -N / -p / -q (src/pmf.h:33-36); the reference-order leg runs without -libpmf_flags.");
            second.libpmf_flags = 0;
        }
        const Stopwatch sw;
        solve_on_gpu(R, T, untouched, second, als);
        printf("[info] reference-order GPU leg training time: %lf s.\n", sw.seconds());
        rule();
        calculate_rmse_directly(untouched.W, untouched.H, T, prm.k, als);
    }

    // The reference compares the -CUDA factors with the -OMP leg's; a leg that did not run leaves its
    // factors at the initial values, and -- exactly like the reference run with one flag only -- the check
    // then reports a mismatch.
    std::cout << "[info] validate the results." << std::endl;
    const long w_outer = als ? R.rows : (long) prm.k, w_inner = als ? (long) prm.k : R.rows;
    const long h_outer = als ? R.cols : (long) prm.k, h_inner = als ? (long) prm.k : R.cols;
    golden_compare(solved.W, untouched.W, w_outer, w_inner);
    golden_compare(solved.H, untouched.H, h_outer, h_inner);

    if (model_path) {
        FILE* fp = fopen(model_path, "wb");
        if (!fp) { fprintf(stderr, "can't open model file %s\n", model_path); return EXIT_FAILURE; }
        // the -CUDA leg's factors (src/main.cpp:146-147 saves W_cuda / H_cuda); with -OMP alone, the reference-order leg's
        const Factors& out = prm.enable_cuda || !prm.enable_omp ? solved : untouched;
        save_mat_t(out.W, fp, als);
        save_mat_t(out.H, fp, als);
        fclose(fp);
        printf("[info] model written to %s\n", model_path);
    }
    rule();
    std::cout << "Total Time: " << whole_run.seconds() << " s.\n";
    return EXIT_SUCCESS;
}
