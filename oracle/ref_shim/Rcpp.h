/*
 * oracle/ref_shim/Rcpp.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Stand-in for the part of Rcpp that the reference's src/cocons_full.cpp, src/cocons_taper.cpp and
 * src/cocons_types.h use, written from Rcpp's documented behaviour so that those three files compile
 * UNMODIFIED without R (oracle/Makefile, target `ref`; tests/r_api_stub/ is the precedent for R's C API).
 * Nothing here is Rcpp's code.  What is provided, and nothing more:
 *   NumericVector   size constructor (zero-filled), [] and (), length() / size(), clone();
 *                   scalar * v, v + v, v - v, v - scalar (elementwise, evaluated once, in that order of
 *                   operations -- Rcpp's lazy sugar evaluates the same expression per element);
 *                   copies SHARE storage, as Rcpp's do; assigning an expression of the same length
 *                   writes into the existing storage (so `idx = idx - 1` changes every copy of idx).
 *   NumericMatrix   (n) square and (nr, nc) constructors (zero-filled, column-major), nrow(),
 *                   (i, j) as an lvalue, (i, _) giving a row that converts to a NumericVector copy.
 *   List            operator[](const char *) giving the stored NumericVector (shared storage).
 *   _               the placeholder of m(i, _).
 */
#ifndef COCONS_REF_SHIM_RCPP_H
#define COCONS_REF_SHIM_RCPP_H

#include <cmath>
#include <cstddef>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace Rcpp {

struct Placeholder {};
static const Placeholder _ = Placeholder();

/* value of an arithmetic expression over vectors: a distinct type, so that assignment can tell
 * `v = expression` (fill v's storage) from `v = w` (share w's storage) */
struct Expression {
    std::vector<double> values;
};

class MatrixRow;

class NumericVector {
    std::shared_ptr<std::vector<double> > d_;
public:
    NumericVector() : d_(std::make_shared<std::vector<double> >()) {}
    explicit NumericVector(int n) : d_(std::make_shared<std::vector<double> >((std::size_t)n, 0.0)) {}
    NumericVector(const double *first, const double *last) : d_(std::make_shared<std::vector<double> >(first, last)) {}
    NumericVector(const Expression &e) : d_(std::make_shared<std::vector<double> >(e.values)) {}
    NumericVector(const MatrixRow &r);
    NumericVector(const NumericVector &) = default;
    NumericVector &operator=(const NumericVector &) = default;
    NumericVector &operator=(const Expression &e)
    {
        if (e.values.size() == d_->size()) *d_ = e.values;
        else d_ = std::make_shared<std::vector<double> >(e.values);
        return *this;
    }
    double &operator[](int i) { return (*d_)[(std::size_t)i]; }
    double &operator()(int i) { return (*d_)[(std::size_t)i]; }
    const double &operator[](int i) const { return (*d_)[(std::size_t)i]; }
    const double &operator()(int i) const { return (*d_)[(std::size_t)i]; }
    int length() const { return (int)d_->size(); }
    int size() const { return (int)d_->size(); }
    const double *begin() const { return d_->data(); }
};

inline NumericVector clone(const NumericVector &v) { return NumericVector(v.begin(), v.begin() + v.size()); }

inline Expression operator*(double s, const NumericVector &v)
{
    Expression e;
    e.values.resize((std::size_t)v.size());
    for (int i = 0; i < v.size(); ++i) e.values[(std::size_t)i] = s * v[i];
    return e;
}

inline Expression operator+(const NumericVector &a, const NumericVector &b)
{
    Expression e;
    e.values.resize((std::size_t)a.size());
    for (int i = 0; i < a.size(); ++i) e.values[(std::size_t)i] = a[i] + b[i];
    return e;
}

inline Expression operator-(const NumericVector &a, const NumericVector &b)
{
    Expression e;
    e.values.resize((std::size_t)a.size());
    for (int i = 0; i < a.size(); ++i) e.values[(std::size_t)i] = a[i] - b[i];
    return e;
}

inline Expression operator-(const NumericVector &a, double s)
{
    Expression e;
    e.values.resize((std::size_t)a.size());
    for (int i = 0; i < a.size(); ++i) e.values[(std::size_t)i] = a[i] - s;
    return e;
}

class NumericMatrix {
    std::shared_ptr<std::vector<double> > d_;
    int nr_, nc_;
public:
    explicit NumericMatrix(int n) : d_(std::make_shared<std::vector<double> >((std::size_t)n * n, 0.0)), nr_(n), nc_(n) {}
    NumericMatrix(int nr, int nc) : d_(std::make_shared<std::vector<double> >((std::size_t)nr * nc, 0.0)), nr_(nr), nc_(nc) {}
    NumericMatrix(int nr, int nc, const double *colmajor)
        : d_(std::make_shared<std::vector<double> >(colmajor, colmajor + (std::size_t)nr * nc)), nr_(nr), nc_(nc) {}
    int nrow() const { return nr_; }
    int ncol() const { return nc_; }
    double &operator()(int i, int j) { return (*d_)[(std::size_t)i + (std::size_t)j * nr_]; }
    const double &operator()(int i, int j) const { return (*d_)[(std::size_t)i + (std::size_t)j * nr_]; }
    MatrixRow operator()(int i, Placeholder) const;
    const double *begin() const { return d_->data(); }
};

class MatrixRow {
    const NumericMatrix &m_;
    int i_;
public:
    MatrixRow(const NumericMatrix &m, int i) : m_(m), i_(i) {}
    int size() const { return m_.ncol(); }
    double operator[](int j) const { return m_(i_, j); }
};

inline MatrixRow NumericMatrix::operator()(int i, Placeholder) const { return MatrixRow(*this, i); }

inline NumericVector::NumericVector(const MatrixRow &r) : d_(std::make_shared<std::vector<double> >((std::size_t)r.size()))
{
    for (int j = 0; j < r.size(); ++j) (*d_)[(std::size_t)j] = r[j];
}

inline Expression operator-(const MatrixRow &a, const MatrixRow &b)
{
    Expression e;
    e.values.resize((std::size_t)a.size());
    for (int j = 0; j < a.size(); ++j) e.values[(std::size_t)j] = a[j] - b[j];
    return e;
}

class List {
    std::map<std::string, NumericVector> items_;
public:
    void set(const char *name, const NumericVector &v) { items_.erase(name); items_.insert(std::make_pair(std::string(name), v)); }
    NumericVector operator[](const char *name) const { return items_.at(name); }
};

}  // namespace Rcpp

#endif
