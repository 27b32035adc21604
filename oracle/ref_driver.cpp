// Driver of the compiled reference (oracle/_ref/insider_ref): reads one case from a directory, calls ONE entry of the
// reference's own translation units (compiled unmodified against oracle/ref_shim), writes the outputs back.
//
//   insider_ref <case directory>
//
// Case directory (oracle/ref.py lays it out and reads it back):
//   manifest.txt      entry <name> | scalar <name> <value> | array <name> <f64|u32> <rows> <cols>   (array data: <name>.bin,
//                     raw little-endian, column-major)
//   out_manifest.txt  the same format, written here
//   log.txt           everything the reference prints to cout (it sets precision 12 in optimize())
//
// Entries: cd, row, col, continuous, state, optimize, selftest.  coordinate_descent (the non-strong solver) is not driven:
// it reads iter_loss before it is first written (src/coordinate_descent.cpp:28).  fit_interaction is compiled but not
// driven: the stand-in refuses its row-view assignment (src/fit_interaction.cpp:54,82).
#include "RcppArmadillo.h"   // the stand-in of oracle/ref_shim (first on the include path)

#include <fstream>
#include <sstream>

using namespace arma;        // the driver's own code names the stand-in's types unqualified, as the reference does

// The reference's functions under our own prototypes: same types, our parameter names; default arguments that the reference
// gives in its definitions are passed explicitly.
typedef const mat& M_in;
typedef const vec& V_in;
typedef const double& D_in;
typedef const int& I_in;
void optimize_row(M_in resid, M_in mask, mat& factor, M_in cf, const uvec& level_of_sample, M_in gram, const double lam, const int tuning,
                  const int threads);
void optimize_col(M_in data, M_in mask, M_in rf, mat& cf, D_in lam, D_in alpha, const int tuning, const int threads, const double tol);
void optimize_continuous_v2(M_in data, M_in mask, rowvec& u, M_in cf, V_in z, M_in gram, const double lam, const int tuning);
Rcpp::List optimize(M_in data, Rcpp::List factors, mat& cf, const umat& levels, M_in ctns, M_in train, M_in test, I_in inc_continuous,
                    const int K, const double lam1, const double lam2, const double alpha, const int tuning, const double global_tol,
                    const double sub_tol, const unsigned int max_iter);
vec strong_coordinate_descent(M_in X, V_in y, V_in w0, D_in lam, D_in alpha, M_in XtX, V_in Xty, D_in tol);
double compute_loss(V_in resid, V_in beta, D_in lam, D_in alpha);
void predict(M_in rf, M_in cf, mat& out);
void evaluate(mat& resid, const uvec& train_idx, const uvec& test_idx, double& sse, double& train_rmse, double& test_rmse, I_in tuning,
              I_in iter, I_in verbose);
double compute_loss(const field<mat>& factors, M_in cf, D_in lam1, D_in lam2, D_in alpha, double& sse, I_in verbose);

namespace {

[[noreturn]] void die(const std::string& msg) {
    std::fflush(stdout);
    std::fprintf(stderr, "insider_ref: %s\n", msg.c_str());
    std::exit(2);
}

struct Case {
    std::string dir, entry;
    std::map<std::string, double> scalars;
    struct Arr { std::string dtype; uword r, c; };
    std::map<std::string, Arr> arrays;
    std::ostringstream out;

    explicit Case(const std::string& d) : dir(d) {
        std::ifstream f((dir + "/manifest.txt").c_str());
        if (!f) die("cannot read " + dir + "/manifest.txt");
        std::string kind;
        while (f >> kind) {
            if (kind == "entry") f >> entry;
            else if (kind == "scalar") { std::string n, v; f >> n >> v; scalars[n] = std::strtod(v.c_str(), nullptr); }
            else if (kind == "array") { std::string n; Arr a; f >> n >> a.dtype >> a.r >> a.c; arrays[n] = a; }
            else die("manifest: unknown record " + kind);
        }
    }
    double s(const std::string& n) const {
        std::map<std::string, double>::const_iterator it = scalars.find(n);
        if (it == scalars.end()) die("manifest: no scalar " + n);
        return it->second;
    }
    bool has(const std::string& n) const { return arrays.count(n) != 0; }
    template <typename T> Mat<T> load(const std::string& n, const char* dtype) const {
        std::map<std::string, Arr>::const_iterator it = arrays.find(n);
        if (it == arrays.end()) die("manifest: no array " + n);
        if (it->second.dtype != dtype) die("array " + n + ": expected dtype " + dtype);
        Mat<T> m(it->second.r, it->second.c);
        std::ifstream f((dir + "/" + n + ".bin").c_str(), std::ios::binary);
        if (!f) die("cannot read array " + n);
        f.read(reinterpret_cast<char*>(m.memptr()), (std::streamsize)(sizeof(T) * (size_t)m.n_elem));
        if ((size_t)f.gcount() != sizeof(T) * (size_t)m.n_elem) die("array " + n + ": file too short");
        return m;
    }
    mat M(const std::string& n) const { return load<double>(n, "f64"); }
    vec V(const std::string& n) const { return vec(M(n)); }
    umat U(const std::string& n) const { return load<uword>(n, "u32"); }
    uvec UV(const std::string& n) const { return uvec(U(n)); }

    template <typename T> void put_raw(const std::string& n, const Mat<T>& m, const char* dtype) {
        std::ofstream f((dir + "/" + n + ".bin").c_str(), std::ios::binary);
        f.write(reinterpret_cast<const char*>(m.memptr()), (std::streamsize)(sizeof(T) * (size_t)m.n_elem));
        if (!f) die("cannot write array " + n);
        out << "array " << n << " " << dtype << " " << m.n_rows << " " << m.n_cols << "\n";
    }
    void put(const std::string& n, const mat& m) { put_raw(n, m, "f64"); }
    void put(const std::string& n, const umat& m) { put_raw(n, m, "u32"); }
    void put(const std::string& n, double v) {
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.17g", v);
        out << "scalar " << n << " " << buf << "\n";
    }
    void finish() {
        put("sweeps", (double)shim_randperm_calls().load());
        std::ofstream f((dir + "/out_manifest.txt").c_str());
        f << out.str();
        if (!f) die("cannot write out_manifest.txt");
    }
};

void run_cd(Case& c) {
    vec beta = strong_coordinate_descent(c.M("X"), c.V("y"), c.V("wstart"), c.s("lambda"), c.s("alpha"), c.M("XtX"), c.V("Xty"),
                                         c.s("tol"));
    c.put("beta", beta);
}

void run_row(Case& c) {
    mat A = c.M("factor");
    optimize_row(c.M("residual"), c.M("indicator"), A, c.M("c_factor"), c.UV("confd"), c.M("gram"), c.s("lambda"), (int)c.s("tuning"),
                 (int)c.s("n_cores"));
    c.put("factor", A);
}

void run_col(Case& c) {
    mat C = c.M("c_factor");
    optimize_col(c.M("residual"), c.M("indicator"), c.M("row_factor"), C, c.s("lambda"), c.s("alpha"), (int)c.s("tuning"),
                 (int)c.s("n_cores"), c.s("tol"));
    c.put("c_factor", C);
}

void run_continuous(Case& c) {
    rowvec u(c.M("u"));
    optimize_continuous_v2(c.M("data"), c.M("indicator"), u, c.M("c_factor"), c.V("confd"), c.M("gram"), c.s("lambda"), (int)c.s("tuning"));
    c.put("u", u);
}

// predict / evaluate / both compute_loss on a fixed state
void run_state(Case& c) {
    cout.precision(12);   // as optimize() sets it before it calls these (src/optimize.cpp:259)
    const int ncfd = (int)c.s("n_factors"), tuning = (int)c.s("tuning");
    field<mat> A(ncfd);
    for (int i = 0; i < ncfd; i++) A(i) = c.M("factor" + std::to_string(i));
    mat C = c.M("column_factor"), R = c.M("row_factor"), data = c.M("data"), pred;
    predict(R, C, pred);
    c.put("predictions", pred);
    mat resid = data - pred;
    uvec tr = find(c.M("train_indicator")), te = find(c.M("test_indicator"));
    double sse = 0.0, trmse = 0.0, termse = 0.0;
    evaluate(resid, tr, te, sse, trmse, termse, tuning, 0, 1);
    c.put("sum_residual", sse);
    c.put("train_rmse", trmse);
    if (tuning == 1) c.put("test_rmse", termse);
    c.put("loss", compute_loss(A, C, c.s("lambda1"), c.s("lambda2"), c.s("alpha"), sse, 1));
    c.put("cd_loss", compute_loss(c.V("cd_residual"), c.V("cd_beta"), c.s("lambda2"), c.s("alpha")));
}

void run_optimize(Case& c) {
    const int ncfd = (int)c.s("n_factors"), tuning = (int)c.s("tuning");
    Rcpp::List factors;
    for (int i = 0; i < ncfd; i++) factors.push_back(c.M("factor" + std::to_string(i)));
    mat C = c.M("column_factor");
    mat ctns = c.has("ctns") ? c.M("ctns") : mat();
    Rcpp::List res = optimize(c.M("data"), factors, C, c.U("levels"), ctns, c.M("train_indicator"), c.M("test_indicator"),
                              (int)c.s("inc_continuous"), (int)c.s("latent_dim"), c.s("lambda1"), c.s("lambda2"), c.s("alpha"), tuning,
                              c.s("global_tol"), c.s("sub_tol"), (unsigned int)c.s("max_iter"));
    Rcpp::List& rows = *res[std::string("row_matrices")].l;
    for (int i = 0; i < ncfd; i++) {
        Rcpp::NumericMatrix m = rows[std::string("factor") + std::to_string(i)];
        c.put("factor" + std::to_string(i), mat(m.begin(), m.nrow(), m.ncol()));
    }
    Rcpp::NumericMatrix cf = res[std::string("column_factor")];
    c.put("column_factor", mat(cf.begin(), cf.nrow(), cf.ncol()));
    c.put("column_factor_arg", C);
    c.put("train_rmse", res[std::string("train_rmse")].s);
    // tuning = 0: the reference returns test_rmse without ever writing it (src/utils.cpp:61-64); it is not recorded
    if (tuning == 1) c.put("test_rmse", res[std::string("test_rmse")].s);
    c.put("loss", res[std::string("loss")].s);
}

// every primitive of the stand-in on arrays from files: tests/test_ref_shim_cpu.py compares each output with numpy
void run_selftest(Case& c) {
    const mat A = c.M("A"), B = c.M("B"), P = c.M("P"), S = c.M("S"), RHS = c.M("RHS"), I = c.M("I");
    const vec v = c.V("v"), w = c.V("w");
    const uvec ri = c.UV("ri"), ci = c.UV("ci"), ei = c.UV("ei"), lv = c.UV("lv");
    const umat Um = c.U("Um");
    const double sc = c.s("sc");
    const uword r0 = (uword)c.s("r0"), c0 = (uword)c.s("c0");
    mat dims(1, 6);
    dims(0) = A.n_rows; dims(1) = A.n_cols; dims(2) = A.n_elem; dims(3) = A.size(); dims(4) = A.is_empty(); dims(5) = mat().is_empty();
    c.put("dims", dims);
    c.put("zeros_rc", zeros(A.n_rows, A.n_cols));
    c.put("zeros_size", zeros(size(A)));
    c.put("zeros_vec", zeros<vec>(v.n_elem));
    c.put("zeros_uvec", zeros<uvec>(v.n_elem));
    c.put("ones_n", ones(v.n_elem));
    c.put("find_I", find(I));
    c.put("find_row_eq0", find(I.row(r0) == 0));
    c.put("find_col_eq0", find(I.col(c0) == 0.0));
    c.put("find_trow", find(trans(I.row(r0))));
    c.put("find_lv_eq", find(lv == lv(0)));
    c.put("find_Um_col_eq", find(Um.col(0) == Um(0, 0)));
    c.put("unique_lv", unique(lv));
    c.put("unique_Um_col", unique(Um.col(0)));
    c.put("lt", abs(v) < sc);
    c.put("gt", abs(v) > sc);
    c.put("trans_A", trans(A));
    c.put("t_A", A.t());
    c.put("trans_v", trans(v));
    c.put("trans_row", trans(A.row(r0)));
    c.put("row_t", A.row(r0).t());
    c.put("sum_v", sum(v));
    c.put("sum_row", sum(A.row(r0)));
    c.put("sum_A_1", vec(sum(A, 1)));
    c.put("sum_A_0", rowvec(sum(A, 0)));
    c.put("sum_sum_abs", sum(sum(abs(A), 1)));
    c.put("accu_A", accu(A));
    c.put("mean_v", mean(v));
    c.put("square_A", square(A));
    c.put("pow_A_2", pow(A, 2));
    c.put("pow_v_2", pow(v, 2));
    c.put("abs_A", abs(A));
    c.put("max_abs_v", max(abs(v)));
    c.put("dot_vw", dot(v, w));
    c.put("dot_col", dot(v, A.col(c0)));
    c.put("norm_A", norm(A, "F"));
    c.put("norm_row", norm(A.row(r0), "F"));
    c.put("as_scalar", as_scalar(trans(v) * A * trans(P.row(0))));
    mat sg(1, 3);
    sg(0) = sign(-2.5); sg(1) = sign(0.0); sg(2) = sign(3.0);
    c.put("sign", sg);
    mat ae(1, 3);
    ae(0) = approx_equal(Um.row(0), Um.row(0), "absdiff", 1e-8);
    ae(1) = approx_equal(Um.row(0), Um.row(1), "absdiff", 1e-8);
    ae(2) = approx_equal(A, A + 1e-9 * B, "absdiff", 1e-8 * (1.0 + max(abs(B))));
    c.put("approx_equal", ae);
    c.put("solve_vec", solve(S, vec(RHS.col(0)), solve_opts::likely_sympd));
    c.put("solve_mat", solve(S, RHS, solve_opts::likely_sympd));
    c.put("randperm", randperm(7));
    c.put("row_r0", A.row(r0));
    c.put("col_c0", A.col(c0));
    c.put("rows_ri", A.rows(ri));
    c.put("cols_ci", A.cols(ci));
    c.put("Um_rows", Um.rows(ri));
    c.put("elem_ei", A.elem(ei));
    c.put("paren_ei", v(ci));
    c.put("sub_ri_ci", A(ri, ci));
    c.put("ei_of_ci", ei(find(ei > 0u)));
    mat at(1, 2);
    at(0) = A(r0 + c0 * A.n_rows); at(1) = A(r0, c0);
    c.put("at", at);
    {   // assignable views
        mat W = A;
        W.row(r0) = 2.0 * A.row(r0);
        W.col(c0) = A.col(c0) - B.col(c0);
        c.put("assign_rowcol", W);
        mat Z = A;
        Z.elem(ei).zeros();
        c.put("elem_zeros", Z);
        vec o = v;
        o(ci).ones();
        o.elem(find(abs(v) > sc)).zeros();
        c.put("elem_ones", o);
        mat D = S;
        D.diag() += sc;
        c.put("diag_plus", D);
        mat F = A;
        F.zeros();
        vec g = v;
        g.ones();
        c.put("zeros_member", F);
        c.put("ones_member", g);
    }
    {   // cube and field
        cube Q(P.n_cols, P.n_cols, P.n_rows);
        for (uword i = 0; i < P.n_rows; i++) Q.slice(i) = P.row(i).t() * P.row(i);
        c.put("cube_sum", sum(Q.slices(ri), 2));
        field<mat> f(2);
        f(0) = A; f(1) = B;
        c.put("field_1", f(1));
    }
    c.put("mat_ptr", mat(A.memptr(), A.n_rows, A.n_cols, false));
    c.put("plus", A + B);
    c.put("minus", A - B);
    c.put("schur", A % B);
    c.put("matmul", A * trans(B));
    c.put("matvec", trans(A) * v);
    c.put("outer", v * trans(w));
    c.put("scal_l", sc * A);
    c.put("scal_r", A * sc);
    c.put("uw_scal", ri.n_elem * A);
    {
        mat X = A; X += B; c.put("plus_eq", X);
        mat Y = A; Y -= sc * B; c.put("minus_eq", Y);
    }
    c.put("uvec_minus_1", lv - 1);
    cout << "selftest " << A.n_rows << endl;
    // Rcpp
    Rcpp::List L;
    L.push_back(A);
    Rcpp::NumericMatrix nm = L[0];
    mat back(nm.begin(), nm.nrow(), nm.ncol(), false);
    Rcpp::List named;
    named["x" + std::to_string(1)] = back;
    Rcpp::List res = Rcpp::List::create(Rcpp::Named("inner") = named, Rcpp::Named("m") = B, Rcpp::Named("d") = sc);
    Rcpp::NumericMatrix x1 = (*res[std::string("inner")].l)[std::string("x1")];
    c.put("rcpp_roundtrip", mat(x1.begin(), x1.nrow(), x1.ncol()));
    c.put("rcpp_scalar", res[std::string("d")].s);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) die("usage: insider_ref <case directory>");
    Case c(argv[1]);
    if (!std::freopen((c.dir + "/log.txt").c_str(), "w", stdout)) die("cannot open log.txt");
    if (c.entry == "cd") run_cd(c);
    else if (c.entry == "row") run_row(c);
    else if (c.entry == "col") run_col(c);
    else if (c.entry == "continuous") run_continuous(c);
    else if (c.entry == "state") run_state(c);
    else if (c.entry == "optimize") run_optimize(c);
    else if (c.entry == "selftest") run_selftest(c);
    else die("unknown entry " + c.entry);
    cout.flush();
    std::fflush(stdout);
    c.finish();
    return 0;
}
