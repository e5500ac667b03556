// The host side of the two-level preconditioner (ehyb_pcg_coarse): aggregates grown inside the partitions of the reordered
// matrix, the coarse matrix E = P^T A P of the piecewise-constant prolongation P, and its dense inverse through a Cholesky
// factorisation.  No GPU is needed here.  Every sum runs in an order that does not depend on the number of OpenMP threads:
// threads share out independent outputs (partitions, rows of E, the entries of a column of L), never the terms of one sum.
// Further down: the vector object (ehyb_coarse_create_host_vecs), whose P holds per aggregate an orthonormal basis of the
// restriction of the caller's near-null-space vectors instead of a constant.
#include <omp.h>

#include <cmath>
#include <numeric>

#include "coarse.h"
#include "ehyb_internal.h"

using namespace ehyb;

namespace {

// the calling thread's OpenMP setting, but never more than the CPUs the process owns
int coarse_threads() { return std::max(1, std::min(omp_get_max_threads(), default_host_threads())); }

// The aggregates of one partition [lo, hi): local numbers 0 .. count - 1 into agg[lo .. hi), by the rules of include/ehyb.h.
int grow_partition(const matrixCOO* m, int lo, int hi, int64_t agg_rows, int32_t* agg)
{
    std::vector<std::vector<int32_t>> members;
    for (int i = lo; i < hi; ++i) agg[i] = -1;
    for (int seed = lo; seed < hi; ++seed) {
        if (agg[seed] >= 0) continue;  // the lowest row not yet in an aggregate
        const int a = (int)members.size();
        members.emplace_back();
        std::vector<int32_t>& q = members.back();
        q.push_back(seed);
        agg[seed] = a;
        for (size_t head = 0; head < q.size() && (int64_t)q.size() < agg_rows; ++head) {
            const int i = q[head];
            for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1] && (int64_t)q.size() < agg_rows; ++e) {
                const int j = m->J[e];
                if (j < lo || j >= hi || agg[j] >= 0) continue;
                agg[j] = a;
                q.push_back(j);
            }
        }
    }
    // fragments: in order of rising size (as grown), ties by number; a fragment is judged by the size it has when its turn comes
    const int na = (int)members.size();
    std::vector<int> order(na);
    std::iota(order.begin(), order.end(), 0);
    std::vector<size_t> grown(na);
    for (int a = 0; a < na; ++a) grown[a] = members[a].size();
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return grown[x] < grown[y]; });
    std::vector<int32_t> votes(na, 0);
    for (int a : order) {
        if (members[a].empty() || 4 * (int64_t)members[a].size() >= agg_rows) continue;
        std::fill(votes.begin(), votes.end(), 0);
        for (int i : members[a])
            for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e) {
                const int j = m->J[e];
                if (j >= lo && j < hi && agg[j] != a) ++votes[agg[j]];
            }
        int best = -1;
        for (int b = 0; b < na; ++b)
            if (votes[b] > 0 && (best < 0 || votes[b] > votes[best])) best = b;
        if (best < 0) continue;  // no neighbour inside the partition: it stays
        for (int i : members[a]) agg[i] = best;
        members[best].insert(members[best].end(), members[a].begin(), members[a].end());
        members[a].clear();
    }
    // the survivors, renumbered in order
    std::vector<int32_t> renum(na, -1);
    int count = 0;
    for (int a = 0; a < na; ++a)
        if (!members[a].empty()) renum[a] = count++;
    for (int i = lo; i < hi; ++i) agg[i] = renum[agg[i]];
    return count;
}

// dot of two rows over [0, len) in a fixed order: eight running sums (index mod 8), added up pairwise at the end
inline double dot_fixed(const double* a, const double* b, int len)
{
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int k = 0;
    for (; k + 8 <= len; k += 8)
        for (int u = 0; u < 8; ++u) s[u] += a[k + u] * b[k + u];
    for (int u = 0; k < len; ++k, ++u) s[u] += a[k] * b[k];
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// E -> E^-1 (both nc x nc, row-major, full): E = L L^T, U = L^-T row by row, E^-1 = U U^T.  false: pivot `bad` is not a
// positive finite number.
bool invert_spd(const std::vector<double>& E, int nc, std::vector<double>* out, int* bad, double* bad_value)
{
    const size_t N = (size_t)nc;
    const int threads = coarse_threads();
    std::vector<double> L(N * N, 0.0), U(N * N, 0.0);
    for (int j = 0; j < nc; ++j) {
        const double* Lj = &L[j * N];
        const double d = E[j * N + j] - dot_fixed(Lj, Lj, j);
        if (!(d > 0) || !std::isfinite(d)) {
            *bad = j;
            *bad_value = d;
            return false;
        }
        const double ljj = std::sqrt(d);
        L[j * N + j] = ljj;
#pragma omp parallel for schedule(static) num_threads(threads) if (nc - j > 256)
        for (int i = j + 1; i < nc; ++i) L[i * N + j] = (E[i * N + j] - dot_fixed(&L[i * N], Lj, j)) / ljj;
    }
    // U[c][i] = (L^-1)[i][c], i >= c: forward substitution on unit vector c; the rows are independent
#pragma omp parallel for schedule(dynamic, 8) num_threads(threads)
    for (int c = 0; c < nc; ++c) {
        double* Uc = &U[c * N];
        Uc[c] = 1.0 / L[c * N + c];
        for (int i = c + 1; i < nc; ++i) Uc[i] = -dot_fixed(&L[i * N + c], Uc + c, i - c) / L[i * N + i];
    }
    // E^-1[c][d] = sum over k >= c of U[c][k] U[d][k] for d <= c, mirrored
    out->assign(N * N, 0.0);
    double* X = out->data();
#pragma omp parallel for schedule(dynamic, 8) num_threads(threads)
    for (int c = 0; c < nc; ++c)
        for (int d = 0; d <= c; ++d) X[c * N + d] = dot_fixed(&U[c * N + c], &U[d * N + c], nc - c);
    for (int c = 0; c < nc; ++c)
        for (int d = 0; d < c; ++d) X[d * N + c] = X[c * N + d];
    return true;
}

int check_matrix(const char* who, const matrixCOO* m)
{
    if (!m || !m->rowIdx || !m->J || !m->V || m->dimension < 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    return EHYB_OK;
}

}  // namespace

bool ehyb::coarse_transpose(ehyb_coarse* c, int groups, int* bad_row, int* empty_unknown)
{
    *bad_row = *empty_unknown = -1;
    c->row_ptr.assign((size_t)groups + 1, 0);
    for (int i = 0; i < c->n; ++i) {
        if (c->map[i] < 0 || c->map[i] >= groups) {
            *bad_row = i;
            return false;
        }
        ++c->row_ptr[c->map[i] + 1];
    }
    for (int u = 0; u < groups; ++u) {
        if (c->row_ptr[u + 1] == 0) {
            *empty_unknown = u;
            return false;
        }
        c->row_ptr[u + 1] += c->row_ptr[u];
    }
    c->rows.resize(c->n);
    std::vector<int32_t> at(c->row_ptr.begin(), c->row_ptr.end() - 1);
    for (int i = 0; i < c->n; ++i) c->rows[at[c->map[i]]++] = i;
    return true;
}

extern "C" int ehyb_coarse_map(const matrixCOO* m, int agg_rows, int dof, int32_t* map_out, int* nc_out)
{
    const char* who = "ehyb_coarse_map";
    clear_error();
    int rc = check_matrix(who, m);
    if (rc != EHYB_OK) return rc;
    if (!map_out || !nc_out) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    if (dof < 1) EHYB_FAIL(EHYB_ERR_ARG, "%s: dof %d (at least 1)", who, dof);
    const int n = m->dimension;
    if (!m->partBoundary || m->nParts < 1 || m->partBoundary[0] != 0 || m->partBoundary[m->nParts] != n)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the matrix has no partition data (call ehyb_matrix_reorder first)", who);
    if (dof > 1 && !m->reorderList) EHYB_FAIL(EHYB_ERR_ARG, "%s: dof %d needs the matrix's reorderList", who, dof);
    const int64_t want = agg_rows > 0 ? agg_rows : std::max<int64_t>(128, ((int64_t)n * dof + 1535) / 1536);

    const int np = m->nParts;
    std::vector<int32_t> agg(std::max(n, 1)), first(np + 1, 0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(coarse_threads())
    for (int p = 0; p < np; ++p) first[p + 1] = grow_partition(m, m->partBoundary[p], m->partBoundary[p + 1], want, agg.data());
    for (int p = 0; p < np; ++p) first[p + 1] += first[p];
    const int64_t n_agg = first[np];
    for (int p = 0; p < np; ++p)
        for (int i = m->partBoundary[p]; i < m->partBoundary[p + 1]; ++i) agg[i] += first[p];

    // the unknown of a row: (aggregate, component of the row before the reorder), the pairs that hold a row numbered in order
    std::vector<int32_t> pair_id;
    int64_t nc = n_agg;
    if (dof > 1) {
        std::vector<int32_t> comp(n);
        for (int old = 0; old < n; ++old) comp[m->reorderList[old]] = old % dof;
        pair_id.assign((size_t)n_agg * dof, 0);
        for (int i = 0; i < n; ++i) pair_id[(size_t)agg[i] * dof + comp[i]] = 1;
        nc = 0;
        for (int32_t& v : pair_id) v = v ? (int32_t)nc++ : -1;
        for (int i = 0; i < n; ++i) agg[i] = pair_id[(size_t)agg[i] * dof + comp[i]];
    }
    if (nc > EHYB_COARSE_MAX)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: %lld coarse unknowns from agg_rows %lld, more than %d: agg_rows %lld would fit", who, (long long)nc,
                  (long long)want, EHYB_COARSE_MAX, (long long)(want * nc / 1536 + 1));
    std::copy(agg.begin(), agg.begin() + n, map_out);
    *nc_out = (int)nc;
    return EHYB_OK;
}

extern "C" int ehyb_coarse_create_host(const matrixCOO* m, const int32_t* map, int nc, ehyb_coarse** out)
{
    const char* who = "ehyb_coarse_create_host";
    clear_error();
    int rc = check_matrix(who, m);
    if (rc != EHYB_OK) return rc;
    if (!map || !out) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    if (nc < 1 || nc > EHYB_COARSE_MAX) EHYB_FAIL(EHYB_ERR_ARG, "%s: %d coarse unknowns (1 .. %d)", who, nc, EHYB_COARSE_MAX);
    std::unique_ptr<ehyb_coarse> c(new (std::nothrow) ehyb_coarse);
    if (!c) EHYB_FAIL(EHYB_ERR_ALLOC, "%s: out of memory", who);
    c->n = m->dimension;
    c->nc = nc;
    c->ld = (nc + 1) & ~1;
    c->map.assign(map, map + c->n);
    int bad_row, empty;
    if (!coarse_transpose(c.get(), nc, &bad_row, &empty)) {
        if (bad_row >= 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: map[%d] = %d is outside 0 .. %d", who, bad_row, map[bad_row], nc - 1);
        EHYB_FAIL(EHYB_ERR_ARG, "%s: coarse unknown %d holds no row", who, empty);
    }
    // E: row u of E takes the entries of u's rows, rows rising and entries in stored order -- one thread per row of E
    const size_t N = (size_t)nc;
    c->E.assign(N * N, 0.0);
    const int threads = coarse_threads();
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads)
    for (int u = 0; u < nc; ++u) {
        double* Eu = &c->E[u * N];
        for (int q = c->row_ptr[u]; q < c->row_ptr[u + 1]; ++q) {
            const int i = c->rows[q];
            for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e) Eu[map[m->J[e]]] += m->V[e];
        }
    }
    // a symmetric matrix stored in full gives E[u][v] and E[v][u] the same terms in two orders: the lower triangle is the one used
    for (int u = 0; u < nc; ++u)
        for (int v = 0; v < u; ++v) c->E[v * N + u] = c->E[u * N + v];
    int bad = -1;
    double bad_value = 0.0;
    if (!invert_spd(c->E, nc, &c->Einv, &bad, &bad_value))
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the coarse matrix is not positive definite (pivot %d of %d is %g)", who, bad, nc, bad_value);
    *out = c.release();
    return EHYB_OK;
}

extern "C" int ehyb_coarse_create_raw(int n, const int32_t* map, int nc, const double* einv, ehyb_coarse** out)
{
    const char* who = "ehyb_coarse_create_raw";
    clear_error();
    if (n < 0 || !map || !einv || !out) EHYB_FAIL(EHYB_ERR_ARG, "%s: bad arguments", who);
    if (nc < 1 || nc > EHYB_COARSE_MAX) EHYB_FAIL(EHYB_ERR_ARG, "%s: %d coarse unknowns (1 .. %d)", who, nc, EHYB_COARSE_MAX);
    std::unique_ptr<ehyb_coarse> c(new (std::nothrow) ehyb_coarse);
    if (!c) EHYB_FAIL(EHYB_ERR_ALLOC, "%s: out of memory", who);
    c->n = n;
    c->nc = nc;
    c->ld = (nc + 1) & ~1;
    c->map.assign(map, map + n);
    int bad_row, empty;
    if (!coarse_transpose(c.get(), nc, &bad_row, &empty)) {
        if (bad_row >= 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: map[%d] = %d is outside 0 .. %d", who, bad_row, map[bad_row], nc - 1);
        EHYB_FAIL(EHYB_ERR_ARG, "%s: coarse unknown %d holds no row", who, empty);
    }
    c->Einv.assign(einv, einv + (size_t)nc * nc);
    *out = c.release();
    return EHYB_OK;
}

// ------------------------------------------------------------------ the vector object: local bases from near-null-space vectors
namespace {

// n, map = agg and its transpose over nagg aggregates; the errors of both vector constructors
int vecs_object(const char* who, int n, const int32_t* agg, int nagg, int nv, std::unique_ptr<ehyb_coarse>* out)
{
    if (nv < 1 || nv > EHYB_COARSE_MAX_VECS) EHYB_FAIL(EHYB_ERR_ARG, "%s: %d vectors (1 .. %d)", who, nv, EHYB_COARSE_MAX_VECS);
    if (nagg < 1) EHYB_FAIL(EHYB_ERR_ARG, "%s: %d aggregates (at least 1)", who, nagg);
    std::unique_ptr<ehyb_coarse> c(new (std::nothrow) ehyb_coarse);
    if (!c) EHYB_FAIL(EHYB_ERR_ALLOC, "%s: out of memory", who);
    c->n = n;
    c->nv = nv;
    c->nagg = nagg;
    c->map.assign(agg, agg + n);
    int bad_row, empty;
    if (!coarse_transpose(c.get(), nagg, &bad_row, &empty)) {
        if (bad_row >= 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: agg[%d] = %d is outside 0 .. %d", who, bad_row, agg[bad_row], nagg - 1);
        EHYB_FAIL(EHYB_ERR_ARG, "%s: aggregate %d holds no row", who, empty);
    }
    *out = std::move(c);
    return EHYB_OK;
}

int vecs_count(const char* who, ehyb_coarse* c, int64_t nc)
{
    if (nc < 1) EHYB_FAIL(EHYB_ERR_ARG, "%s: no column was kept in any aggregate: 0 coarse unknowns (1 .. %d)", who, EHYB_COARSE_MAX);
    if (nc > EHYB_COARSE_MAX)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: %lld coarse unknowns from %d aggregates and %d vectors, more than %d: fewer aggregates or vectors are needed",
                  who, (long long)nc, c->nagg, c->nv, EHYB_COARSE_MAX);
    c->nc = (int)nc;
    c->ld = (c->nc + 1) & ~1;
    return EHYB_OK;
}

// The local basis of one aggregate (rows idx[0 .. len), rising): columns 0 .. nv - 1 of B in turn, each orthogonalised against
// the columns kept so far by modified Gram-Schmidt, two passes, and kept iff it is not zero and at least kCut of it is left.
// Q: nv * len doubles of the caller's, the kept columns in order.  -> the number kept
constexpr double kCut = EHYB_COARSE_VEC_CUT;
int local_basis(const double* B, int64_t ldb, int nv, const int32_t* idx, int len, double* Q)
{
    int kept = 0;
    for (int v = 0; v < nv; ++v) {
        double* t = Q + (size_t)kept * len;
        for (int q = 0; q < len; ++q) t[q] = B[(size_t)v * ldb + idx[q]];
        const double norm0 = std::sqrt(dot_fixed(t, t, len));
        if (!(norm0 > 0)) continue;
        for (int pass = 0; pass < 2; ++pass)
            for (int k = 0; k < kept; ++k) {
                const double* Qk = Q + (size_t)k * len;
                const double h = dot_fixed(Qk, t, len);
                for (int q = 0; q < len; ++q) t[q] -= h * Qk[q];
            }
        const double norm1 = std::sqrt(dot_fixed(t, t, len));
        if (!(norm1 >= kCut * norm0)) continue;
        for (int q = 0; q < len; ++q) t[q] /= norm1;
        ++kept;
    }
    return kept;
}

}  // namespace

extern "C" int ehyb_coarse_create_host_vecs(const matrixCOO* m, const int32_t* agg, int nagg, const double* B, int64_t ldb, int nv,
                                            ehyb_coarse** out)
{
    const char* who = "ehyb_coarse_create_host_vecs";
    clear_error();
    int rc = check_matrix(who, m);
    if (rc != EHYB_OK) return rc;
    if (!agg || !B || !out) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    const int n = m->dimension;
    if (ldb < n) EHYB_FAIL(EHYB_ERR_ARG, "%s: ldb %lld is below the %d rows", who, (long long)ldb, n);
    std::unique_ptr<ehyb_coarse> c;
    if ((rc = vecs_object(who, n, agg, nagg, nv, &c)) != EHYB_OK) return rc;
    for (int v = 0; v < nv; ++v)
        for (int i = 0; i < n; ++i)
            if (!std::isfinite(B[(size_t)v * ldb + i]))
                EHYB_FAIL(EHYB_ERR_ARG, "%s: B holds %g in row %d of column %d", who, B[(size_t)v * ldb + i], i, v);

    // the local bases: one thread per aggregate, every sum inside one thread
    const int threads = coarse_threads();
    const size_t N0 = (size_t)n;
    c->W.assign((size_t)nv * N0, 0.0);
    c->off.assign((size_t)nagg + 1, 0);
#pragma omp parallel num_threads(threads)
    {
        std::vector<double> Q;
#pragma omp for schedule(dynamic, 4)
        for (int a = 0; a < nagg; ++a) {
            const int begin = c->row_ptr[a], len = c->row_ptr[a + 1] - begin;
            Q.assign((size_t)nv * len, 0.0);
            const int kept = local_basis(B, ldb, nv, &c->rows[begin], len, Q.data());
            c->off[a + 1] = kept;
            for (int j = 0; j < kept; ++j)
                for (int q = 0; q < len; ++q) c->W[j * N0 + c->rows[begin + q]] = Q[(size_t)j * len + q];
        }
    }
    int64_t total = 0;
    for (int a = 0; a < nagg; ++a) total += c->off[a + 1];
    if ((rc = vecs_count(who, c.get(), total)) != EHYB_OK) return rc;
    for (int a = 0; a < nagg; ++a) c->off[a + 1] += c->off[a];

    // E = P^T A P.  Row (a, j) of E takes the rows i of aggregate a, rising, and their entries in stored order: the entry a_ic
    // adds (W_j[i] a_ic) W_j'[c] to column (agg[c], j'), j' rising over the kept columns there.  One thread per aggregate.
    const int nc = c->nc;
    const size_t N = (size_t)nc;
    c->E.assign(N * N, 0.0);
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads)
    for (int a = 0; a < nagg; ++a)
        for (int j = 0; j < c->off[a + 1] - c->off[a]; ++j) {
            double* Eu = &c->E[(size_t)(c->off[a] + j) * N];
            const double* Wj = &c->W[j * N0];
            for (int q = c->row_ptr[a]; q < c->row_ptr[a + 1]; ++q) {
                const int i = c->rows[q];
                for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e) {
                    const int col = m->J[e], b = agg[col];
                    const double wa = Wj[i] * m->V[e];
                    for (int o = c->off[b], j2 = 0; o < c->off[b + 1]; ++o, ++j2) Eu[o] += wa * c->W[j2 * N0 + col];
                }
            }
        }
    for (int u = 0; u < nc; ++u)
        for (int v = 0; v < u; ++v) c->E[v * N + u] = c->E[u * N + v];
    int bad = -1;
    double bad_value = 0.0;
    if (!invert_spd(c->E, nc, &c->Einv, &bad, &bad_value))
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the coarse matrix is not positive definite (pivot %d of %d is %g)", who, bad, nc, bad_value);
    *out = c.release();
    return EHYB_OK;
}

extern "C" int ehyb_coarse_create_raw_vecs(int n, const int32_t* agg, int nagg, const int32_t* off, const double* W, int64_t ldw, int nv,
                                           const double* einv, ehyb_coarse** out)
{
    const char* who = "ehyb_coarse_create_raw_vecs";
    clear_error();
    if (n < 0 || !agg || !off || !W || !einv || !out) EHYB_FAIL(EHYB_ERR_ARG, "%s: bad arguments", who);
    if (ldw < n) EHYB_FAIL(EHYB_ERR_ARG, "%s: ldw %lld is below the %d rows", who, (long long)ldw, n);
    std::unique_ptr<ehyb_coarse> c;
    int rc = vecs_object(who, n, agg, nagg, nv, &c);
    if (rc != EHYB_OK) return rc;
    if (off[0] != 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: off[0] = %d, not 0", who, off[0]);
    for (int a = 0; a < nagg; ++a)
        if (off[a + 1] < off[a] || off[a + 1] - off[a] > nv)
            EHYB_FAIL(EHYB_ERR_ARG, "%s: aggregate %d keeps %d columns (0 .. %d)", who, a, off[a + 1] - off[a], nv);
    c->off.assign(off, off + nagg + 1);
    if ((rc = vecs_count(who, c.get(), off[nagg])) != EHYB_OK) return rc;
    c->W.resize((size_t)nv * n);
    for (int j = 0; j < nv; ++j) std::copy(W + (size_t)j * ldw, W + (size_t)j * ldw + n, &c->W[(size_t)j * n]);
    c->Einv.assign(einv, einv + (size_t)c->nc * c->nc);
    *out = c.release();
    return EHYB_OK;
}

extern "C" int ehyb_coarse_host_array(const ehyb_coarse* c, int which, const void** ptr, int64_t* count)
{
    clear_error();
    if (!c || !ptr || !count) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_coarse_host_array: null argument");
    switch (which) {
    case EHYB_COARSE_MAP: *ptr = c->map.data(), *count = (int64_t)c->map.size(); break;
    case EHYB_COARSE_ROW_PTR: *ptr = c->row_ptr.data(), *count = (int64_t)c->row_ptr.size(); break;
    case EHYB_COARSE_ROWS: *ptr = c->rows.data(), *count = (int64_t)c->rows.size(); break;
    case EHYB_COARSE_E: *ptr = c->E.data(), *count = (int64_t)c->E.size(); break;
    case EHYB_COARSE_EINV: *ptr = c->Einv.data(), *count = (int64_t)c->Einv.size(); break;
    case EHYB_COARSE_OFF:
    case EHYB_COARSE_W:
        if (!c->nv) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_coarse_host_array: no array %d on an object without vectors", which);
        if (which == EHYB_COARSE_OFF)
            *ptr = c->off.data(), *count = (int64_t)c->off.size();
        else
            *ptr = c->W.data(), *count = (int64_t)c->W.size();
        break;
    default: EHYB_FAIL(EHYB_ERR_ARG, "ehyb_coarse_host_array: no array %d", which);
    }
    return EHYB_OK;
}
