// Stand-in for <RcppArmadillo.h>: the slice of Armadillo and Rcpp that the reference's four translation units use,
// written here from the libraries' documented behaviour so that those units compile unmodified without R.
//
// Rules ("The compiled reference"):
//   * eager value types, column-major, every access bounds-checked; no expression templates, no BLAS/LAPACK;
//   * each primitive is the plainest correct loop in double;
//   * solve(A, B, solve_opts::likely_sympd) is a Cholesky solve and aborts where Cholesky fails;
//   * where Armadillo's behaviour is not certain the stand-in aborts with a message naming the construct
//     (REFUSE below) instead of guessing;
//   * randperm(n) returns 0..n-1 (the cyclic sweep order, order_mode = 1) and counts its calls;
//   * .row/.col/.elem views are copies that remember their parent and write through on assignment; they are safe
//     under the reference's OpenMP loops because those write disjoint rows/columns.
#ifndef INSIDER_REF_SHIM_RCPPARMADILLO_H
#define INSIDER_REF_SHIM_RCPPARMADILLO_H

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace arma {

using std::cout;
using std::endl;

typedef unsigned int uword;   // RcppArmadillo builds with 32-bit words

[[noreturn]] inline void shim_die(const char* kind, const char* what) {
    std::fflush(stdout);
    std::fprintf(stderr, "ref_shim %s: %s\n", kind, what);
    std::fflush(stderr);
    std::abort();
}
#define SHIM_CHECK(cond, what) do { if (!(cond)) ::arma::shim_die("check failed", what); } while (0)
#define REFUSE(what) ::arma::shim_die("refuses", what)

// one call of randperm is one sweep of a coordinate-descent loop: the driver reads the reference's own sweep count here
inline std::atomic<unsigned long long>& shim_randperm_calls() {
    static std::atomic<unsigned long long> n(0);
    return n;
}

struct SizeMat { uword n_rows, n_cols; };
struct solve_opts { struct opts {}; static constexpr opts likely_sympd = opts(); };

template <typename T> class Col;
template <typename T> class Row;
template <typename T> class subview_row;
template <typename T> class subview_col;
template <typename T> class subview_elem;
template <typename T> class diagview;

template <typename T>
class Mat {
public:
    typedef T elem_type;
    uword n_rows, n_cols, n_elem;
    std::vector<T> mem;

    Mat() : n_rows(0), n_cols(0), n_elem(0) {}
    Mat(uword r, uword c) : n_rows(r), n_cols(c), n_elem(r * c), mem((size_t)r * c, T(0)) {}
    // mat(ptr, r, c, false): Armadillo would alias the caller's buffer; the stand-in copies it.  The reference reads its
    // results from the returned List (src/optimize.cpp:413), so the aliasing is not observable through the driver.
    Mat(const T* p, uword r, uword c, bool /*copy_aux_mem*/ = true) : n_rows(r), n_cols(c), n_elem(r * c), mem(p, p + (size_t)r * c) {}

    void set_size(uword r, uword c) { n_rows = r; n_cols = c; n_elem = r * c; mem.assign((size_t)r * c, T(0)); }
    uword size() const { return n_elem; }
    bool is_empty() const { return n_elem == 0; }
    const T* memptr() const { return mem.data(); }
    T* memptr() { return mem.data(); }

    T& operator()(uword i) { SHIM_CHECK(i < n_elem, "Mat::operator()(i): index out of bounds"); return mem[i]; }
    const T& operator()(uword i) const { SHIM_CHECK(i < n_elem, "Mat::operator()(i): index out of bounds"); return mem[i]; }
    T& operator()(uword i, uword j) { SHIM_CHECK(i < n_rows && j < n_cols, "Mat::operator()(i,j): index out of bounds"); return mem[(size_t)j * n_rows + i]; }
    const T& operator()(uword i, uword j) const { SHIM_CHECK(i < n_rows && j < n_cols, "Mat::operator()(i,j): index out of bounds"); return mem[(size_t)j * n_rows + i]; }

    Mat& zeros() { std::fill(mem.begin(), mem.end(), T(0)); return *this; }
    Mat& ones() { std::fill(mem.begin(), mem.end(), T(1)); return *this; }

    subview_row<T> row(uword i) { return subview_row<T>(this, this, i); }
    subview_row<T> row(uword i) const { return subview_row<T>(this, nullptr, i); }
    subview_col<T> col(uword j) { return subview_col<T>(this, this, j); }
    subview_col<T> col(uword j) const { return subview_col<T>(this, nullptr, j); }

    Mat rows(const Col<uword>& idx) const;
    Mat cols(const Col<uword>& idx) const;
    subview_elem<T> elem(const Col<uword>& idx);
    subview_elem<T> elem(const Col<uword>& idx) const;
    subview_elem<T> operator()(const Col<uword>& idx);
    subview_elem<T> operator()(const Col<uword>& idx) const;
    Mat operator()(const Col<uword>& ri, const Col<uword>& ci) const;
    diagview<T> diag() { return diagview<T>(this); }

    Mat t() const {
        Mat out(n_cols, n_rows);
        for (uword j = 0; j < n_cols; j++) for (uword i = 0; i < n_rows; i++) out(j, i) = (*this)(i, j);
        return out;
    }

    Mat& operator+=(const Mat& b) {
        SHIM_CHECK(n_rows == b.n_rows && n_cols == b.n_cols, "operator+=: incompatible sizes");
        for (size_t i = 0; i < mem.size(); i++) mem[i] += b.mem[i];
        return *this;
    }
    Mat& operator-=(const Mat& b) {
        SHIM_CHECK(n_rows == b.n_rows && n_cols == b.n_cols, "operator-=: incompatible sizes");
        for (size_t i = 0; i < mem.size(); i++) mem[i] -= b.mem[i];
        return *this;
    }
};

template <typename T>
class Col : public Mat<T> {
public:
    Col() : Mat<T>() { this->n_cols = 1; }
    explicit Col(uword n) : Mat<T>(n, 1) {}
    explicit Col(const Mat<T>& m) : Mat<T>(m) { SHIM_CHECK(m.n_cols == 1 || m.n_elem == 0, "Col from Mat: not a column"); this->n_cols = 1; this->n_rows = m.n_elem; }
    Col& operator=(const Mat<T>& m) { SHIM_CHECK(m.n_cols == 1 || m.n_elem == 0, "Col = Mat: not a column"); Mat<T>::operator=(m); this->n_cols = 1; this->n_rows = m.n_elem; return *this; }
    Row<T> t() const;
};

template <typename T>
class Row : public Mat<T> {
public:
    Row() : Mat<T>() { this->n_rows = 1; }
    explicit Row(uword n) : Mat<T>(1, n) {}
    explicit Row(const Mat<T>& m) : Mat<T>(m) { SHIM_CHECK(m.n_rows == 1 || m.n_elem == 0, "Row from Mat: not a row"); this->n_rows = 1; this->n_cols = m.n_elem; }
    Row& operator=(const Mat<T>& m) { SHIM_CHECK(m.n_rows == 1 || m.n_elem == 0, "Row = Mat: not a row"); Mat<T>::operator=(m); this->n_rows = 1; this->n_cols = m.n_elem; return *this; }
    Col<T> t() const;
};

template <typename T> Row<T> Col<T>::t() const { Row<T> r(this->n_elem); r.mem = this->mem; return r; }
template <typename T> Col<T> Row<T>::t() const { Col<T> c(this->n_elem); c.mem = this->mem; return c; }

// ---- views: a copy of the selected elements plus the parent to write through to -------------------------------------
template <typename T>
class subview_row : public Row<T> {
    Mat<T>* wr; uword idx;
public:
    subview_row(const Mat<T>* src, Mat<T>* w, uword i) : Row<T>(src->n_cols), wr(w), idx(i) {
        SHIM_CHECK(i < src->n_rows, "Mat::row(): index out of bounds");
        for (uword j = 0; j < src->n_cols; j++) this->mem[j] = (*src)(i, j);
    }
    subview_row(const subview_row&) = default;
    void store(const Mat<T>& v) {
        SHIM_CHECK(wr != nullptr, "assignment to a row of a const matrix");
        SHIM_CHECK(v.n_rows == 1 && v.n_cols == wr->n_cols, "row view = : incompatible sizes");
        for (uword j = 0; j < wr->n_cols; j++) (*wr)(idx, j) = v.mem[j];
        this->mem = v.mem;
    }
    subview_row& operator=(const Row<T>& v) { store(v); return *this; }
    subview_row& operator=(const Mat<T>& v) { store(v); return *this; }
    subview_row& operator=(const subview_row& v) { store(v); return *this; }
    subview_row& operator=(const Col<T>& v) {
        // src/fit_interaction.cpp:54,82 assigns the K x 1 result of solve() to a 1 x K row view
        (void)v; REFUSE("assigning a column vector to a row view (dimension mismatch in Armadillo unless K = 1)");
    }
};

template <typename T>
class subview_col : public Col<T> {
    Mat<T>* wr; uword idx;
public:
    subview_col(const Mat<T>* src, Mat<T>* w, uword j) : Col<T>(src->n_rows), wr(w), idx(j) {
        SHIM_CHECK(j < src->n_cols, "Mat::col(): index out of bounds");
        for (uword i = 0; i < src->n_rows; i++) this->mem[i] = (*src)(i, j);
    }
    subview_col(const subview_col&) = default;
    void store(const Mat<T>& v) {
        SHIM_CHECK(wr != nullptr, "assignment to a column of a const matrix");
        SHIM_CHECK(v.n_cols == 1 && v.n_rows == wr->n_rows, "column view = : incompatible sizes");
        for (uword i = 0; i < wr->n_rows; i++) (*wr)(i, idx) = v.mem[i];
        this->mem = v.mem;
    }
    subview_col& operator=(const Col<T>& v) { store(v); return *this; }
    subview_col& operator=(const Mat<T>& v) { store(v); return *this; }
    subview_col& operator=(const subview_col& v) { store(v); return *this; }
};

template <typename T>
class subview_elem : public Col<T> {
    Mat<T>* wr; Col<uword> ids;
public:
    subview_elem(const Mat<T>* src, Mat<T>* w, const Col<uword>& idx) : Col<T>(idx.n_elem), wr(w), ids(idx) {
        for (uword k = 0; k < idx.n_elem; k++) {
            SHIM_CHECK(idx.mem[k] < src->n_elem, "elem(): index out of bounds");
            this->mem[k] = src->mem[idx.mem[k]];
        }
    }
    void fill(T v) {
        SHIM_CHECK(wr != nullptr, "write through elem() of a const object");
        for (uword k = 0; k < ids.n_elem; k++) { wr->mem[ids.mem[k]] = v; this->mem[k] = v; }
    }
    void zeros() { fill(T(0)); }
    void ones() { fill(T(1)); }
};

template <typename T>
class diagview {
    Mat<T>* m;
public:
    explicit diagview(Mat<T>* p) : m(p) {}
    void operator+=(T s) { uword n = std::min(m->n_rows, m->n_cols); for (uword i = 0; i < n; i++) (*m)(i, i) += s; }
};

template <typename T> Mat<T> Mat<T>::rows(const Col<uword>& idx) const {
    Mat out(idx.n_elem, n_cols);
    for (uword j = 0; j < n_cols; j++) for (uword k = 0; k < idx.n_elem; k++) out(k, j) = (*this)(idx(k), j);
    return out;
}
template <typename T> Mat<T> Mat<T>::cols(const Col<uword>& idx) const {
    Mat out(n_rows, idx.n_elem);
    for (uword k = 0; k < idx.n_elem; k++) for (uword i = 0; i < n_rows; i++) out(i, k) = (*this)(i, idx(k));
    return out;
}
template <typename T> subview_elem<T> Mat<T>::elem(const Col<uword>& idx) { return subview_elem<T>(this, this, idx); }
template <typename T> subview_elem<T> Mat<T>::elem(const Col<uword>& idx) const { return subview_elem<T>(this, nullptr, idx); }
template <typename T> subview_elem<T> Mat<T>::operator()(const Col<uword>& idx) { return elem(idx); }
template <typename T> subview_elem<T> Mat<T>::operator()(const Col<uword>& idx) const { return elem(idx); }
template <typename T> Mat<T> Mat<T>::operator()(const Col<uword>& ri, const Col<uword>& ci) const {
    Mat out(ri.n_elem, ci.n_elem);
    for (uword b = 0; b < ci.n_elem; b++) for (uword a = 0; a < ri.n_elem; a++) out(a, b) = (*this)(ri(a), ci(b));
    return out;
}

typedef Mat<double> mat;
typedef Col<double> vec;
typedef Row<double> rowvec;
typedef Mat<uword> umat;
typedef Col<uword> uvec;
typedef Row<uword> urowvec;

// ---- cube and field -----------------------------------------------------------------------------------------------
class cube {
public:
    uword n_rows, n_cols, n_slices;
    std::vector<mat> s;
    class slice_ref {
        mat* m;
    public:
        explicit slice_ref(mat* p) : m(p) {}
        slice_ref& operator=(const mat& v) {
            SHIM_CHECK(v.n_rows == m->n_rows && v.n_cols == m->n_cols, "cube.slice() = : incompatible sizes");
            m->mem = v.mem;
            return *this;
        }
        operator const mat&() const { return *m; }
    };
    cube() : n_rows(0), n_cols(0), n_slices(0) {}
    cube(uword r, uword c, uword n) : n_rows(r), n_cols(c), n_slices(n), s(n, mat(r, c)) {}
    slice_ref slice(uword i) { SHIM_CHECK(i < n_slices, "cube.slice(): index out of bounds"); return slice_ref(&s[i]); }
    const mat& slice(uword i) const { SHIM_CHECK(i < n_slices, "cube.slice(): index out of bounds"); return s[i]; }
    cube slices(const uvec& idx) const {
        cube out(n_rows, n_cols, 0);
        for (uword k = 0; k < idx.n_elem; k++) {
            SHIM_CHECK(idx(k) < n_slices, "cube.slices(): index out of bounds");
            out.s.push_back(s[idx(k)]);
        }
        out.n_slices = idx.n_elem;
        return out;
    }
};

template <typename T>
class field {
    std::vector<T> v;
public:
    uword n_elem;
    field() : n_elem(0) {}
    explicit field(uword n) : v(n), n_elem(n) {}
    T& operator()(uword i) { SHIM_CHECK(i < n_elem, "field(): index out of bounds"); return v[i]; }
    const T& operator()(uword i) const { SHIM_CHECK(i < n_elem, "field(): index out of bounds"); return v[i]; }
};

// ---- generators ---------------------------------------------------------------------------------------------------
inline mat zeros(uword r, uword c) { return mat(r, c); }
inline mat zeros(const SizeMat& s) { return mat(s.n_rows, s.n_cols); }
template <typename V> inline V zeros(uword n) { return V(n); }
inline vec ones(uword n) { vec v(n); v.ones(); return v; }
template <typename T> inline SizeMat size(const Mat<T>& X) { SizeMat s = {X.n_rows, X.n_cols}; return s; }
inline uvec randperm(uword n) {
    shim_randperm_calls().fetch_add(1, std::memory_order_relaxed);
    uvec p(n);
    for (uword i = 0; i < n; i++) p.mem[i] = i;
    return p;
}

// ---- find, unique, relational operators ---------------------------------------------------------------------------
template <typename T> inline uvec find(const Mat<T>& X) {
    uword cnt = 0;
    for (uword i = 0; i < X.n_elem; i++) cnt += (X.mem[i] != T(0));
    uvec out(cnt);
    uword k = 0;
    for (uword i = 0; i < X.n_elem; i++) if (X.mem[i] != T(0)) out.mem[k++] = i;
    return out;
}
template <typename T> inline Col<T> unique(const Mat<T>& X) {
    std::vector<T> v(X.mem);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    Col<T> out((uword)v.size());
    out.mem = v;
    return out;
}
#define SHIM_REL(OP)                                                                                        \
    template <typename T, typename S>                                                                       \
    inline typename std::enable_if<std::is_arithmetic<S>::value, umat>::type operator OP(const Mat<T>& X, S s) { \
        umat out(X.n_rows, X.n_cols);                                                                       \
        for (uword i = 0; i < X.n_elem; i++) out.mem[i] = (X.mem[i] OP (T)s) ? 1u : 0u;                      \
        return out;                                                                                         \
    }
SHIM_REL(==)
SHIM_REL(<)
SHIM_REL(>)
#undef SHIM_REL

template <typename T> inline bool approx_equal(const Mat<T>& a, const Mat<T>& b, const char* method, double tol) {
    SHIM_CHECK(std::strcmp(method, "absdiff") == 0, "approx_equal: only \"absdiff\" is provided");
    if (a.n_rows != b.n_rows || a.n_cols != b.n_cols) return false;
    for (uword i = 0; i < a.n_elem; i++) {
        double d = (double)a.mem[i] - (double)b.mem[i];
        if (!(std::fabs(d) <= tol)) return false;
    }
    return true;
}

// ---- transposes ---------------------------------------------------------------------------------------------------
inline mat trans(const mat& X) { return X.t(); }
inline rowvec trans(const vec& X) { return X.t(); }
inline vec trans(const rowvec& X) { return X.t(); }
inline umat trans(const umat& X) { return X.t(); }

// ---- element-wise arithmetic: one overload per shape so that vectors stay vectors -----------------------------------
#define SHIM_EW2(NAME, EXPR, TYPE)                                                                 \
    inline TYPE NAME(const TYPE& A, const TYPE& B) {                                               \
        SHIM_CHECK(A.n_rows == B.n_rows && A.n_cols == B.n_cols, #NAME ": incompatible sizes");    \
        TYPE out(A);                                                                               \
        for (uword i = 0; i < A.n_elem; i++) { double a = A.mem[i], b = B.mem[i]; out.mem[i] = (EXPR); } \
        return out;                                                                                \
    }
#define SHIM_EW2_ALL(NAME, EXPR) SHIM_EW2(NAME, EXPR, mat) SHIM_EW2(NAME, EXPR, vec) SHIM_EW2(NAME, EXPR, rowvec)
SHIM_EW2_ALL(operator+, a + b)
SHIM_EW2_ALL(operator-, a - b)
SHIM_EW2_ALL(operator%, a * b)
#undef SHIM_EW2_ALL
#undef SHIM_EW2

#define SHIM_EW1(NAME, EXPR, TYPE)                                                                 \
    inline TYPE NAME(const TYPE& A) {                                                              \
        TYPE out(A);                                                                               \
        for (uword i = 0; i < A.n_elem; i++) { double a = A.mem[i]; out.mem[i] = (EXPR); }         \
        return out;                                                                                \
    }
#define SHIM_EW1_ALL(NAME, EXPR) SHIM_EW1(NAME, EXPR, mat) SHIM_EW1(NAME, EXPR, vec) SHIM_EW1(NAME, EXPR, rowvec)
SHIM_EW1_ALL(square, a * a)
SHIM_EW1_ALL(abs, std::fabs(a))
#undef SHIM_EW1_ALL
#undef SHIM_EW1

#define SHIM_SC(TYPE)                                                                                                   \
    inline TYPE operator*(double s, const TYPE& A) { TYPE out(A); for (uword i = 0; i < A.n_elem; i++) out.mem[i] = s * A.mem[i]; return out; } \
    inline TYPE operator*(const TYPE& A, double s) { TYPE out(A); for (uword i = 0; i < A.n_elem; i++) out.mem[i] = A.mem[i] * s; return out; } \
    inline TYPE pow(const TYPE& A, double e) {                                                                          \
        SHIM_CHECK(e == 2.0, "pow(X, e): only e = 2 is provided");                                                      \
        TYPE out(A); for (uword i = 0; i < A.n_elem; i++) out.mem[i] = A.mem[i] * A.mem[i]; return out;                 \
    }
SHIM_SC(mat) SHIM_SC(vec) SHIM_SC(rowvec)
#undef SHIM_SC

inline uvec operator-(const uvec& A, uword s) {
    uvec out(A);
    for (uword i = 0; i < A.n_elem; i++) { SHIM_CHECK(A.mem[i] >= s, "uvec - s: result below zero"); out.mem[i] = A.mem[i] - s; }
    return out;
}

// ---- matrix product: C(i,j) = sum_k A(i,k) B(k,j), k ascending ----------------------------------------------------
inline void shim_mul(const mat& A, const mat& B, mat& out) {
    SHIM_CHECK(A.n_cols == B.n_rows, "operator*: incompatible sizes");
    for (uword j = 0; j < B.n_cols; j++)
        for (uword i = 0; i < A.n_rows; i++) {
            double acc = 0.0;
            for (uword k = 0; k < A.n_cols; k++) acc += A.mem[(size_t)k * A.n_rows + i] * B.mem[(size_t)j * B.n_rows + k];
            out.mem[(size_t)j * A.n_rows + i] = acc;
        }
}
inline mat operator*(const mat& A, const mat& B) { mat out(A.n_rows, B.n_cols); shim_mul(A, B, out); return out; }
inline vec operator*(const mat& A, const vec& B) { vec out(A.n_rows); shim_mul(A, B, out); return out; }
inline rowvec operator*(const rowvec& A, const mat& B) { rowvec out(B.n_cols); shim_mul(A, B, out); return out; }
inline mat operator*(const rowvec& A, const vec& B) { mat out(1, 1); shim_mul(A, B, out); return out; }

// ---- reductions: plain left-to-right sums -------------------------------------------------------------------------
inline double accu(const mat& X) { double s = 0.0; for (uword i = 0; i < X.n_elem; i++) s += X.mem[i]; return s; }
inline double sum(const vec& X) { return accu(X); }
inline double sum(const rowvec& X) { return accu(X); }
// sum(M, dim): dim 0 gives the column sums as a row, dim 1 the row sums as a column.  sum(sum(M, dim)) is the sum of
// all elements (Armadillo detects the two consecutive calls and returns a scalar).
class SumOut : public mat {
public:
    SumOut(uword r, uword c) : mat(r, c) {}
    operator vec() const { return vec(static_cast<const mat&>(*this)); }
    operator rowvec() const { return rowvec(static_cast<const mat&>(*this)); }
};
inline SumOut sum(const mat& X, uword dim) {
    SHIM_CHECK(dim <= 1, "sum(M, dim): dim must be 0 or 1");
    SumOut out(dim == 0 ? 1 : X.n_rows, dim == 0 ? X.n_cols : 1);
    for (uword j = 0; j < X.n_cols; j++)
        for (uword i = 0; i < X.n_rows; i++) out.mem[dim == 0 ? j : i] += X.mem[(size_t)j * X.n_rows + i];
    return out;
}
inline double sum(const SumOut& X) { return accu(X); }
inline mat sum(const cube& Q, uword dim) {
    SHIM_CHECK(dim == 2, "sum(cube, dim): only dim = 2 is provided");
    // src/optimize.cpp:218 reaches this with no slice when a column of the training indicator has no zero
    if (Q.n_slices == 0) REFUSE("sum(cube.slices(idx), 2) with an empty index selection");
    mat out(Q.n_rows, Q.n_cols);
    for (uword k = 0; k < Q.n_slices; k++) out += Q.s[k];
    return out;
}
inline double mean(const mat& X) {
    if (X.n_elem == 0) REFUSE("mean() of an object with no elements");
    return accu(X) / (double)X.n_elem;
}
inline double max(const mat& X) {
    if (X.n_elem == 0) REFUSE("max() of an object with no elements");
    double m = X.mem[0];
    for (uword i = 1; i < X.n_elem; i++) if (X.mem[i] > m) m = X.mem[i];
    return m;
}
inline double dot(const mat& A, const mat& B) {
    SHIM_CHECK(A.n_elem == B.n_elem, "dot(): incompatible sizes");
    double s = 0.0;
    for (uword i = 0; i < A.n_elem; i++) s += A.mem[i] * B.mem[i];
    return s;
}
inline double norm(const mat& X, const char* method) {
    SHIM_CHECK(std::strcmp(method, "F") == 0 || std::strcmp(method, "fro") == 0, "norm(): only \"F\" is provided");
    double s = 0.0;
    for (uword i = 0; i < X.n_elem; i++) s += X.mem[i] * X.mem[i];
    return std::sqrt(s);
}
inline double as_scalar(const mat& X) { SHIM_CHECK(X.n_elem == 1, "as_scalar(): not 1 x 1"); return X.mem[0]; }
inline double sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// ---- solve(A, B, likely_sympd): Cholesky A = L L', forward and back substitution -----------------------------------
inline void shim_chol_solve(const mat& A, const mat& B, mat& X) {
    SHIM_CHECK(A.n_rows == A.n_cols, "solve(): A is not square");
    SHIM_CHECK(A.n_rows == B.n_rows, "solve(): incompatible sizes");
    const uword n = A.n_rows;
    mat L(n, n);
    for (uword j = 0; j < n; j++) {
        double d = A(j, j);
        for (uword k = 0; k < j; k++) d -= L(j, k) * L(j, k);
        if (!(d > 0.0)) REFUSE("solve(..., likely_sympd) of a matrix that is not positive definite (Armadillo's fallback solvers are not imitated)");
        d = std::sqrt(d);
        L(j, j) = d;
        for (uword i = j + 1; i < n; i++) {
            double v = A(i, j);
            for (uword k = 0; k < j; k++) v -= L(i, k) * L(j, k);
            L(i, j) = v / d;
        }
    }
    for (uword c = 0; c < B.n_cols; c++) {
        for (uword i = 0; i < n; i++) {
            double v = B(i, c);
            for (uword k = 0; k < i; k++) v -= L(i, k) * X(k, c);
            X(i, c) = v / L(i, i);
        }
        for (uword ii = n; ii-- > 0;) {
            double v = X(ii, c);
            for (uword k = ii + 1; k < n; k++) v -= L(k, ii) * X(k, c);
            X(ii, c) = v / L(ii, ii);
        }
    }
}
inline mat solve(const mat& A, const mat& B, solve_opts::opts) { mat X(B.n_rows, B.n_cols); shim_chol_solve(A, B, X); return X; }
inline vec solve(const mat& A, const vec& B, solve_opts::opts) { vec X(B.n_rows); shim_chol_solve(A, B, X); return X; }

}  // namespace arma

// ---- Rcpp: List, Named, NumericMatrix -----------------------------------------------------------------------------
namespace Rcpp {

class NumericMatrix {
    std::shared_ptr<std::vector<double> > d;
    int r, c;
public:
    NumericMatrix() : d(new std::vector<double>()), r(0), c(0) {}
    NumericMatrix(const arma::mat& m) : d(new std::vector<double>(m.mem)), r((int)m.n_rows), c((int)m.n_cols) {}
    double* begin() { return d->data(); }
    const double* begin() const { return d->data(); }
    int nrow() const { return r; }
    int ncol() const { return c; }
};

class List;

class Value {
public:
    enum Kind { NONE, MATRIX, SCALAR, LIST } kind;
    NumericMatrix m;
    double s;
    std::shared_ptr<List> l;
    Value() : kind(NONE), s(0.0) {}
    Value(const arma::mat& x) : kind(MATRIX), m(x), s(0.0) {}
    Value(double x) : kind(SCALAR), s(x) {}
    Value(const List& x);
    Value& operator=(const arma::mat& x) { kind = MATRIX; m = NumericMatrix(x); return *this; }
    operator NumericMatrix() const { if (kind != MATRIX) arma::shim_die("check failed", "List element is not a matrix"); return m; }
};

struct NamedValue { std::string name; Value value; };
class Named {
    std::string name;
public:
    explicit Named(const std::string& n) : name(n) {}
    template <typename V> NamedValue operator=(const V& v) const { NamedValue nv; nv.name = name; nv.value = Value(v); return nv; }
};

class List {
public:
    std::vector<std::pair<std::string, Value> > items;
    List() {}
    Value& operator[](size_t i) { if (i >= items.size()) arma::shim_die("check failed", "List[i]: index out of bounds"); return items[i].second; }
    Value& operator[](int i) { return (*this)[(size_t)i]; }
    Value& operator[](unsigned int i) { return (*this)[(size_t)i]; }
    Value& operator[](const std::string& name) {
        for (size_t i = 0; i < items.size(); i++) if (items[i].first == name) return items[i].second;
        items.push_back(std::make_pair(name, Value()));
        return items.back().second;
    }
    void push_back(const arma::mat& m, const std::string& name = "") { items.push_back(std::make_pair(name, Value(m))); }
    template <typename... Args> static List create(const Args&... args) {
        List out;
        NamedValue all[] = {args...};
        for (size_t i = 0; i < sizeof...(Args); i++) out.items.push_back(std::make_pair(all[i].name, all[i].value));
        return out;
    }
};

inline Value::Value(const List& x) : kind(LIST), s(0.0), l(new List(x)) {}

}  // namespace Rcpp

#endif
