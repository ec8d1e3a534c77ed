// libpyslam_hipvol.so — pose-graph optimisation (hv_pose_graph_optimize, hv_pose_graph_linearise; contract in include/hipvol.h).
//
// Levenberg-Marquardt over the node poses with a block-Jacobi preconditioned conjugate-gradient inner solve.  The matrix is never
// formed: an edge keeps M_e = J_s^T (l Omega) J_s (upper triangle, 21 doubles) and g_e = J_s^T (l Omega) r, struct-of-arrays so
// that a wave's loads coalesce; a product H p is one pass over the edges (u_e = M_e (p_s - p_t)) and one over the nodes (the node
// adds +u_e / -u_e down its incidence list, a CSR sorted by edge index that the host builds once per call).  Every sum over edges
// or nodes has two stages in a fixed order - lanes by butterfly, waves in order, workgroups in order - and there is no float
// atomic, so a call is bitwise reproducible.  alpha, beta and the CG's "done" flag live on the device (PgState, the CG scalars
// double-buffered by iteration parity so that no kernel reads what another workgroup of the same launch writes): a finished CG
// turns the rest of its queued launches into no-ops, and an outer iteration costs ONE host wait - the read of the state behind its
// decide kernel.  At the sizes this runs at the call is bound by its launch count (7 + 4 cg_max_iterations per outer iteration), not
// by bandwidth.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "hv_common.h"
#include "hv_lm.h"

namespace {
// One edge at the poses T: r, chi2, l, and - where asked for - M_e and g_e.  One lane per edge.  part_F[workgroup] = the
// workgroup's sum of l chi2 + mu (sqrt(l) - 1)^2.  kept (may be null): the count of l >= thr.
__global__ __launch_bounds__(PG_BLOCK) void k_pg_linearise(const double *__restrict__ T, const int32_t *__restrict__ nodes,
                                                            const double *__restrict__ Zs, const double *__restrict__ info,
                                                            const uint8_t *__restrict__ unc, int E, double mu, double *__restrict__ M21,
                                                            double *__restrict__ g_out, double *__restrict__ r_out, double *__restrict__ chi_out,
                                                            double *__restrict__ l_out, double *__restrict__ part_F, double thr,
                                                            PgState *__restrict__ S, int count_kept) {
    __shared__ double red[4];
    const int e = blockIdx.x * PG_BLOCK + threadIdx.x;
    double cost = 0.0;
    if (e < E) {
        const int s = nodes[2 * e], t = nodes[2 * e + 1];
        const double *Ts = T + (size_t)s * 16, *Tt = T + (size_t)t * 16, *Z = Zs + (size_t)e * 16;
        // A = inv(T_t) = [Ra, ta];  B = T_s inv(Z) = [Rb, tb];  X = A B
        double Ra[9], ta[3], Rb[9], tb[3], Rx[9], r[6];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Ra[i * 3 + j] = Tt[j * 4 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) ta[i] = -((Ra[i * 3] * Tt[3] + Ra[i * 3 + 1] * Tt[7]) + Ra[i * 3 + 2] * Tt[11]);
        {
            double zi[3]; // the translation of inv(Z)
#pragma unroll
            for (int i = 0; i < 3; ++i) zi[i] = -((Z[i] * Z[3] + Z[4 + i] * Z[7]) + Z[8 + i] * Z[11]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) Rb[i * 3 + j] = (Ts[i * 4] * Z[j * 4] + Ts[i * 4 + 1] * Z[j * 4 + 1]) + Ts[i * 4 + 2] * Z[j * 4 + 2];
                tb[i] = ((Ts[i * 4] * zi[0] + Ts[i * 4 + 1] * zi[1]) + Ts[i * 4 + 2] * zi[2]) + Ts[i * 4 + 3];
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Rx[i * 3 + j] = (Ra[i * 3] * Rb[j] + Ra[i * 3 + 1] * Rb[3 + j]) + Ra[i * 3 + 2] * Rb[6 + j];
            r[3 + i] = ((Ra[i * 3] * tb[0] + Ra[i * 3 + 1] * tb[1]) + Ra[i * 3 + 2] * tb[2]) + ta[i];
        }
        pg_log_rot(Rx, r);
        double Om[36];
#pragma unroll
        for (int k = 0; k < 36; ++k) Om[k] = info[(size_t)e * 36 + k];
        double Or[6], chi = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double q = 0.0;
#pragma unroll
            for (int b = 0; b < 6; ++b) q += Om[a * 6 + b] * r[b];
            Or[a] = q;
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) chi += r[a] * Or[a];
        double l = 1.0;
        if (unc != nullptr && unc[e] != 0) {
            const double q = mu / (mu + chi);
            l = q * q;
            const double d = sqrt(l) - 1.0;
            cost = l * chi + mu * (d * d);
        } else {
            cost = chi;
        }
        if (r_out != nullptr)
#pragma unroll
            for (int a = 0; a < 6; ++a) r_out[(size_t)a * E + e] = r[a];
        if (chi_out != nullptr) chi_out[e] = chi;
        if (l_out != nullptr) l_out[e] = l;
        if (count_kept && l >= thr) atomicAdd(&S->kept, 1); // an integer count: order-free
        if (M21 != nullptr) {
            // J_s = [[Jw Ra, 0], [[ta - t]x Ra, Ra]],  Jw = I - K / 2 + c2 K^2,  K = [omega]x
            const double w0 = r[0], w1 = r[1], w2 = r[2];
            const double th2 = (w0 * w0 + w1 * w1) + w2 * w2, th = sqrt(th2);
            double c2;
            if (th < PG_JINV_SERIES) {
                c2 = 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0));
            } else {
                const double h = 0.5 * th;
                c2 = 1.0 / th2 - cos(h) / (2.0 * th * sin(h));
            }
            const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
            double Jw[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double kk = (K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j]) + K[i * 3 + 2] * K[6 + j];
                    Jw[i * 3 + j] = ((i == j ? 1.0 : 0.0) - 0.5 * K[i * 3 + j]) + c2 * kk;
                }
            const double d0 = ta[0] - r[3], d1 = ta[1] - r[4], d2 = ta[2] - r[5];
            const double Dx[9] = {0.0, -d2, d1, d2, 0.0, -d0, -d1, d0, 0.0};
            double J[36];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    J[i * 6 + j] = (Jw[i * 3] * Ra[j] + Jw[i * 3 + 1] * Ra[3 + j]) + Jw[i * 3 + 2] * Ra[6 + j];
                    J[i * 6 + 3 + j] = 0.0;
                    J[(3 + i) * 6 + j] = (Dx[i * 3] * Ra[j] + Dx[i * 3 + 1] * Ra[3 + j]) + Dx[i * 3 + 2] * Ra[6 + j];
                    J[(3 + i) * 6 + 3 + j] = Ra[i * 3 + j];
                }
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                double wj[6];
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    double q = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) q += Om[a * 6 + k] * J[k * 6 + b];
                    wj[a] = q;
                }
#pragma unroll
                for (int a = 0; a <= b; ++a) {
                    double q = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) q += J[k * 6 + a] * wj[k];
                    M21[(size_t)pg_tri(a, b) * E + e] = l * q;
                }
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double q = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) q += J[k * 6 + a] * Or[k];
                g_out[(size_t)a * E + e] = l * q;
            }
        }
    }
    const double tot = pg_block_sum(cost, red);
    if (threadIdx.x == 0 && part_F != nullptr) part_F[blockIdx.x] = tot;
}

// One lane per node: D_i = sum of M_e and b_i = sum of +g_e (source) / -g_e (target) down the incidence list; the fixed node gets
// b = 0.  part_maxd / part_grad[workgroup]: the largest diagonal entry of D and the largest |b| of the workgroup's free nodes.
__global__ __launch_bounds__(PG_BLOCK) void k_pg_gather(const int32_t *__restrict__ row, const int32_t *__restrict__ ent,
                                                         const double *__restrict__ M21, const double *__restrict__ g, int N, int E, int fixed,
                                                         double *__restrict__ D21, double *__restrict__ b, double *__restrict__ part_maxd,
                                                         double *__restrict__ part_grad) {
    __shared__ double red[4];
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    double maxd = 0.0, maxg = 0.0;
    if (i < N) {
        double D[21], bb[6];
#pragma unroll
        for (int q = 0; q < 21; ++q) D[q] = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) bb[a] = 0.0;
        for (int k = row[i]; k < row[i + 1]; ++k) {
            const int e = ent[k] >> 1;
            const double sg = (ent[k] & 1) ? -1.0 : 1.0;
#pragma unroll
            for (int q = 0; q < 21; ++q) D[q] += M21[(size_t)q * E + e];
#pragma unroll
            for (int a = 0; a < 6; ++a) bb[a] += sg * g[(size_t)a * E + e];
        }
#pragma unroll
        for (int q = 0; q < 21; ++q) D21[(size_t)q * N + i] = D[q];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double v = i == fixed ? 0.0 : bb[a];
            b[(size_t)a * N + i] = v;
            maxg = fmax(maxg, fabs(v));
            if (i != fixed) maxd = fmax(maxd, D[pg_tri(a, a)]);
        }
    }
    const double md = pg_block_max(maxd, red), mg = pg_block_max(maxg, red);
    if (threadIdx.x == 0) part_maxd[blockIdx.x] = md, part_grad[blockIdx.x] = mg;
}

// One lane per node: lambda (the first iteration takes lambda_scale max diag H), the Cholesky factor of D_i + lambda I, and the start
// of the CG: x = 0, r = -b, z = P^-1 r, part_rz.
__global__ __launch_bounds__(PG_BLOCK) void k_pg_factor(PgState *__restrict__ S, const double *__restrict__ part_maxd, int nbN,
                                                         double lambda_scale, const double *__restrict__ D21, const double *__restrict__ b,
                                                         int N, int fixed, double *__restrict__ L21, double *__restrict__ x,
                                                         double *__restrict__ rr, double *__restrict__ z, double *__restrict__ part_rz) {
    __shared__ double red[4];
    __shared__ double sh;
    double lambda;
    if (S->iter == 0) {
        if (threadIdx.x == 0) {
            double m = 0.0;
            for (int k = 0; k < nbN; ++k) m = fmax(m, part_maxd[k]);
            sh = lambda_scale * m;
        }
        __syncthreads();
        lambda = sh;
        if (blockIdx.x == 0 && threadIdx.x == 0) S->lambda = lambda;
    } else {
        lambda = S->lambda;
    }
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    double rz = 0.0;
    if (i < N) {
        double A[21], L[21];
#pragma unroll
        for (int q = 0; q < 21; ++q) A[q] = D21[(size_t)q * N + i];
        bool bad = pg_chol6(A, lambda, L);
        if (i == fixed) {
            bad = false;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = a; c < 6; ++c) L[pg_tri(a, c)] = a == c ? 1.0 : 0.0;
        }
        if (bad) atomicOr(&S->bad, 1);
#pragma unroll
        for (int q = 0; q < 21; ++q) L21[(size_t)q * N + i] = L[q];
        double r6[6], z6[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) r6[a] = -b[(size_t)a * N + i];
        pg_precond(L, r6, z6);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            x[(size_t)a * N + i] = 0.0;
            rr[(size_t)a * N + i] = r6[a];
            z[(size_t)a * N + i] = z6[a];
            rz += r6[a] * z6[a];
        }
    }
    const double tot = pg_block_sum(rz, red);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = tot;
}

// second: u_e = M_e (p_s - p_t), one lane per edge
__global__ __launch_bounds__(PG_BLOCK) void k_pg_cg_edges(const PgState *__restrict__ S, int j, const int32_t *__restrict__ nodes,
                                                           const double *__restrict__ M21, int E, int N, const double *__restrict__ p,
                                                           double *__restrict__ u) {
    if (S->done[j & 1]) return;
    const int e = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int s = nodes[2 * e], t = nodes[2 * e + 1];
    double d[6], M[21];
#pragma unroll
    for (int a = 0; a < 6; ++a) d[a] = p[(size_t)a * N + s] - p[(size_t)a * N + t];
#pragma unroll
    for (int q = 0; q < 21; ++q) M[q] = M21[(size_t)q * E + e];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double q = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) q += M[a <= c ? pg_tri(a, c) : pg_tri(c, a)] * d[c];
        u[(size_t)a * E + e] = q;
    }
}

// third: q_i = lambda p_i + sum of +u_e / -u_e down the incidence list (0 for the fixed node), part_pq
__global__ __launch_bounds__(PG_BLOCK) void k_pg_cg_nodes(const PgState *__restrict__ S, int j, const int32_t *__restrict__ row,
                                                           const int32_t *__restrict__ ent, const double *__restrict__ u, int N, int E, int fixed,
                                                           const double *__restrict__ p, double *__restrict__ qv, double *__restrict__ part_pq) {
    __shared__ double red[4];
    if (S->done[j & 1]) return;
    const double lambda = S->lambda;
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    double pq = 0.0;
    if (i < N) {
        double acc[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] = lambda * p[(size_t)a * N + i];
        for (int k = row[i]; k < row[i + 1]; ++k) {
            const int e = ent[k] >> 1;
            const double sg = (ent[k] & 1) ? -1.0 : 1.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[a] += sg * u[(size_t)a * E + e];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double v = i == fixed ? 0.0 : acc[a];
            qv[(size_t)a * N + i] = v;
            pq += p[(size_t)a * N + i] * v;
        }
    }
    const double tot = pg_block_sum(pq, red);
    if (threadIdx.x == 0) part_pq[blockIdx.x] = tot;
}

struct PgFind { // union-find over the nodes (host)
    std::vector<int32_t> up;
    explicit PgFind(int n) : up((size_t)n) { std::iota(up.begin(), up.end(), 0); }
    int root(int a) {
        while (up[(size_t)a] != a) a = up[(size_t)a] = up[(size_t)up[(size_t)a]];
        return a;
    }
    void join(int a, int b) { up[(size_t)root(a)] = root(b); }
};

bool pg_rigid_row(const double *T) {
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T[i])) return false;
    return T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0;
}

// The host's checks of the graph, before any launch.  connected: also that every node reaches `fixed` through certain edges.
int pg_check_graph(const char *fn, const double *poses, int64_t N, const int32_t *nodes, const double *Zs, const double *info,
                   const uint8_t *unc, int64_t E, int fixed, bool connected) {
    for (int64_t i = 0; i < N; ++i)
        HV_REQUIRE(pg_rigid_row(poses + i * 16), HV_ERR_INVALID, "%s: pose %lld is not finite or its bottom row is not 0 0 0 1", fn, (long long)i);
    for (int64_t e = 0; e < E; ++e) {
        const int s = nodes[2 * e], t = nodes[2 * e + 1];
        HV_REQUIRE(s >= 0 && s < N && t >= 0 && t < N, HV_ERR_INVALID, "%s: edge %lld joins nodes %d and %d, outside 0..%lld", fn, (long long)e, s, t,
                   (long long)N - 1);
        HV_REQUIRE(s != t, HV_ERR_INVALID, "%s: edge %lld joins node %d to itself", fn, (long long)e, s);
        HV_REQUIRE(pg_rigid_row(Zs + e * 16), HV_ERR_INVALID, "%s: the transformation of edge %lld is not finite or its bottom row is not 0 0 0 1", fn,
                   (long long)e);
        const double *Om = info + e * 36;
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b)
                HV_REQUIRE(std::isfinite(Om[a * 6 + b]) && Om[a * 6 + b] == Om[b * 6 + a], HV_ERR_INVALID,
                           "%s: the information matrix of edge %lld is not finite or not symmetric (bitwise)", fn, (long long)e);
    }
    if (connected) {
        PgFind uf((int)N);
        for (int64_t e = 0; e < E; ++e)
            if (unc == nullptr || unc[e] == 0) uf.join(nodes[2 * e], nodes[2 * e + 1]);
        const int root = uf.root(fixed);
        for (int64_t i = 0; i < N; ++i)
            HV_REQUIRE(uf.root((int)i) == root, HV_ERR_INVALID,
                       "%s: node %lld is not connected to the fixed node %d through certain edges (union-find over the edges that are not "
                       "uncertain): the line process could cut it loose",
                       fn, (long long)i, fixed);
    }
    return HV_OK;
}

// the operands on the host, for the checks and the incidence list: the caller's arrays (HV_HOST) or copies (HV_DEVICE; one wait)
struct PgHostView {
    std::vector<double> poses, Z, info;
    std::vector<int32_t> nodes;
    std::vector<uint8_t> unc;
    const double *p_poses, *p_Z, *p_info;
    const int32_t *p_nodes;
    const uint8_t *p_unc;
};
int pg_host_view(hv_volume *v, PgHostView &h, const double *poses, int64_t N, const int32_t *nodes, const double *Z, const double *info,
                 const uint8_t *unc, int64_t E, int32_t loc) {
    h.p_poses = poses, h.p_nodes = nodes, h.p_Z = Z, h.p_info = info, h.p_unc = unc;
    if (loc == HV_HOST) return HV_OK;
    h.poses.resize((size_t)N * 16), h.nodes.resize((size_t)E * 2), h.Z.resize((size_t)E * 16), h.info.resize((size_t)E * 36);
    HV_HIP(hipMemcpyAsync(h.poses.data(), poses, sizeof(double) * 16 * (size_t)N, hipMemcpyDeviceToHost, v->stream));
    if (E > 0) {
        HV_HIP(hipMemcpyAsync(h.nodes.data(), nodes, sizeof(int32_t) * 2 * (size_t)E, hipMemcpyDeviceToHost, v->stream));
        HV_HIP(hipMemcpyAsync(h.Z.data(), Z, sizeof(double) * 16 * (size_t)E, hipMemcpyDeviceToHost, v->stream));
        HV_HIP(hipMemcpyAsync(h.info.data(), info, sizeof(double) * 36 * (size_t)E, hipMemcpyDeviceToHost, v->stream));
        if (unc != nullptr) {
            h.unc.resize((size_t)E);
            HV_HIP(hipMemcpyAsync(h.unc.data(), unc, (size_t)E, hipMemcpyDeviceToHost, v->stream));
        }
    }
    HV_HIP(hipStreamSynchronize(v->stream));
    h.p_poses = h.poses.data(), h.p_nodes = h.nodes.data(), h.p_Z = h.Z.data(), h.p_info = h.info.data();
    h.p_unc = unc != nullptr ? h.unc.data() : nullptr;
    return HV_OK;
}

// row [N + 1] and ent [2 E]: node i's entries (edge << 1 | is-target) in the order of the edge index
void pg_incidence(const int32_t *nodes, int64_t N, int64_t E, std::vector<int32_t> &csr) {
    csr.assign((size_t)(N + 1 + 2 * E), 0);
    int32_t *row = csr.data(), *ent = csr.data() + N + 1;
    for (int64_t e = 0; e < E; ++e) row[nodes[2 * e] + 1]++, row[nodes[2 * e + 1] + 1]++;
    for (int64_t i = 0; i < N; ++i) row[i + 1] += row[i];
    std::vector<int32_t> at(row, row + N);
    for (int64_t e = 0; e < E; ++e) {
        ent[at[(size_t)nodes[2 * e]]++] = (int32_t)(e << 1);
        ent[at[(size_t)nodes[2 * e + 1]]++] = (int32_t)(e << 1) | 1;
    }
}

constexpr int64_t PG_MAX_NODES = 1 << 22, PG_MAX_EDGES = 1 << 24;
} // namespace

extern "C" void hv_pose_graph_default_params(hv_pose_graph_params *p) {
    if (p == nullptr) return;
    p->line_process_weight = 1.0;
    p->edge_prune_threshold = 0.25;
    p->lambda_scale = 1.0e-5;
    p->gradient_tolerance = 1.0e-6;
    p->step_tolerance = 1.0e-6;
    p->decrease_tolerance = 1.0e-6;
    p->residual_tolerance = 1.0e-6;
    p->cg_tolerance = 1.0e-8;
    p->max_iterations = 100;
    p->cg_max_iterations = 100;
    p->fixed = 0;
    p->trace_state = 0;
}

extern "C" int hv_pose_graph_optimize(hv_volume *v, double *poses, int64_t n_nodes, const int32_t *edge_nodes, const double *edge_T,
                                      const double *edge_info, const uint8_t *edge_uncertain, int64_t n_edges,
                                      const hv_pose_graph_params *prm, double *edge_weight_out, hv_pose_graph_result *res, double *trace,
                                      double *trace_poses, int64_t trace_cap, int64_t *trace_rows, int32_t loc) {
    const char *fn = "hv_pose_graph_optimize";
    HV_REQUIRE(v != nullptr && prm != nullptr && res != nullptr, HV_ERR_INVALID, "%s: null argument", fn);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    const int64_t N = n_nodes, E = n_edges;
    HV_REQUIRE(N >= 1 && N <= PG_MAX_NODES, HV_ERR_INVALID, "%s: need 1 .. %lld nodes, got %lld", fn, (long long)PG_MAX_NODES, (long long)N);
    HV_REQUIRE(E >= 0 && E <= PG_MAX_EDGES, HV_ERR_INVALID, "%s: need 0 .. %lld edges, got %lld", fn, (long long)PG_MAX_EDGES, (long long)E);
    HV_REQUIRE(poses != nullptr && (E == 0 || (edge_nodes != nullptr && edge_T != nullptr && edge_info != nullptr)), HV_ERR_INVALID,
               "%s: null poses or edge arrays", fn);
    HV_REQUIRE(prm->fixed >= 0 && prm->fixed < N, HV_ERR_INVALID, "%s: the fixed node %d is outside 0..%lld", fn, (int)prm->fixed, (long long)N - 1);
    HV_REQUIRE(std::isfinite(prm->line_process_weight) && prm->line_process_weight > 0.0, HV_ERR_INVALID,
               "%s: line_process_weight must be positive and finite", fn);
    HV_REQUIRE(prm->edge_prune_threshold >= 0.0 && prm->edge_prune_threshold <= 1.0, HV_ERR_INVALID, "%s: edge_prune_threshold must be in 0..1", fn);
    HV_REQUIRE(std::isfinite(prm->lambda_scale) && prm->lambda_scale > 0.0, HV_ERR_INVALID, "%s: lambda_scale must be positive and finite", fn);
    HV_REQUIRE(prm->gradient_tolerance >= 0.0 && prm->step_tolerance >= 0.0 && prm->decrease_tolerance >= 0.0 && prm->residual_tolerance >= 0.0 &&
                   prm->cg_tolerance >= 0.0 && prm->cg_tolerance < 1.0,
               HV_ERR_INVALID, "%s: a tolerance is negative (or cg_tolerance is not below 1)", fn);
    HV_REQUIRE(prm->max_iterations >= 1 && prm->max_iterations <= 10000 && prm->cg_max_iterations >= 1 && prm->cg_max_iterations <= 10000,
               HV_ERR_INVALID, "%s: max_iterations and cg_max_iterations must be in 1..10000", fn);
    HV_REQUIRE(trace == nullptr || trace_cap >= 0, HV_ERR_INVALID, "%s: negative trace_cap", fn);
    HV_REQUIRE(!prm->trace_state || (trace != nullptr && trace_poses != nullptr), HV_ERR_INVALID, "%s: trace_state needs trace and trace_poses", fn);
    HV_HIP(hipSetDevice(v->device));

    PgHostView h;
    int rc = pg_host_view(v, h, poses, N, edge_nodes, edge_T, edge_info, edge_uncertain, E, loc);
    if (rc != HV_OK) return rc;
    rc = pg_check_graph(fn, h.p_poses, N, h.p_nodes, h.p_Z, h.p_info, h.p_unc, E, prm->fixed, true);
    if (rc != HV_OK) return rc;
    if (trace_rows) *trace_rows = 0;
    memset(res, 0, sizeof(*res));
    if (E == 0) { // N == 1 (the connectivity check): nothing to move
        res->success = 1;
        res->converged = HV_POSE_GRAPH_GRADIENT;
        return HV_OK;
    }
    std::vector<int32_t> csr;
    pg_incidence(h.p_nodes, N, E, csr);

    const int nbE = (int)((E + PG_BLOCK - 1) / PG_BLOCK), nbN = (int)((N + PG_BLOCK - 1) / PG_BLOCK);
    const int cap = trace != nullptr ? (int)std::min<int64_t>(trace_cap, prm->max_iterations) : 0;
    const int cap_state = prm->trace_state ? cap : 0;
    PgLayout lay;
    const size_t o_state = lay.take(sizeof(PgState));
    const size_t o_T = lay.take(128 * (size_t)N), o_Tn = lay.take(128 * (size_t)N);
    const size_t o_csr = lay.take(4 * csr.size());
    const size_t o_M = lay.take(8 * 21 * (size_t)E), o_g = lay.take(8 * 6 * (size_t)E), o_u = lay.take(8 * 6 * (size_t)E);
    const size_t o_l = lay.take(8 * (size_t)E);
    const size_t o_D = lay.take(8 * 21 * (size_t)N), o_L = lay.take(8 * 21 * (size_t)N);
    size_t o_vec[6]; // b, x, r, z, p, q
    for (size_t &o : o_vec) o = lay.take(8 * 6 * (size_t)N);
    size_t o_partN[6]; // maxd, grad, rz, pq, dd, pred
    for (size_t &o : o_partN) o = lay.take(8 * (size_t)nbN);
    const size_t o_pF = lay.take(8 * (size_t)nbE), o_pFn = lay.take(8 * (size_t)nbE);
    const size_t o_trace = lay.take(8 * HV_POSE_GRAPH_TRACE_STRIDE * (size_t)std::max(cap, 1));
    const size_t o_tstate = lay.take(128 * (size_t)N * (size_t)cap_state);
    rc = hv_ensure_buffer(v, &v->track_buf, &v->track_buf_bytes, lay.off);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->track_buf;
    PgState *S = (PgState *)(base + o_state);
    double *T = (double *)(base + o_T), *Tn = (double *)(base + o_Tn);
    int32_t *d_row = (int32_t *)(base + o_csr), *d_ent = d_row + N + 1;
    double *M21 = (double *)(base + o_M), *g = (double *)(base + o_g), *u = (double *)(base + o_u), *d_l = (double *)(base + o_l);
    double *D21 = (double *)(base + o_D), *L21 = (double *)(base + o_L);
    double *b = (double *)(base + o_vec[0]), *x = (double *)(base + o_vec[1]), *rr = (double *)(base + o_vec[2]);
    double *z = (double *)(base + o_vec[3]), *p = (double *)(base + o_vec[4]), *qv = (double *)(base + o_vec[5]);
    double *p_maxd = (double *)(base + o_partN[0]), *p_grad = (double *)(base + o_partN[1]), *p_rz = (double *)(base + o_partN[2]);
    double *p_pq = (double *)(base + o_partN[3]), *p_dd = (double *)(base + o_partN[4]), *p_pred = (double *)(base + o_partN[5]);
    double *p_F = (double *)(base + o_pF), *p_Fn = (double *)(base + o_pFn);
    double *d_trace = (double *)(base + o_trace), *d_tstate = (double *)(base + o_tstate);

    HvStage st(v, loc);
    const int i_pin = st.in(poses, 128 * (size_t)N), i_nodes = st.in(edge_nodes, 8 * (size_t)E), i_Z = st.in(edge_T, 128 * (size_t)E);
    const int i_info = st.in(edge_info, 288 * (size_t)E), i_unc = st.in(edge_uncertain, (size_t)E);
    const int i_pout = st.out(poses, 128 * (size_t)N), i_w = st.out(edge_weight_out, 8 * (size_t)E);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    const int32_t *d_nodes = st.dev<const int32_t>(i_nodes);
    const double *d_Z = st.dev<const double>(i_Z), *d_info = st.dev<const double>(i_info);
    const uint8_t *d_unc = st.dev<const uint8_t>(i_unc);
    double *d_w = st.dev<double>(i_w);
    v->pipe_armed = false; // as hv_rgbd_odometry: the next batch starts a fresh chain behind this call

    PgState h0{};
    h0.nu = 2.0;
    HV_HIP(hipMemcpyAsync(S, &h0, sizeof(PgState), hipMemcpyHostToDevice, v->stream));
    HV_HIP(hipMemcpyAsync(d_row, csr.data(), 4 * csr.size(), hipMemcpyHostToDevice, v->stream));
    HV_HIP(hipMemcpyAsync(T, st.dev<const double>(i_pin), 128 * (size_t)N, hipMemcpyDeviceToDevice, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream)); // h0 and csr are host memory of this frame

    const double mu = prm->line_process_weight, tol2 = prm->cg_tolerance * prm->cg_tolerance;
    const PgRules rules{prm->gradient_tolerance, prm->step_tolerance, prm->decrease_tolerance, prm->residual_tolerance, prm->max_iterations};
    const int fixed = prm->fixed;
    const dim3 gE((unsigned)nbE), gN((unsigned)nbN), blk(PG_BLOCK);
    const int64_t n16 = 16 * N;
    PgState hs{};
    for (int it = 0; it < prm->max_iterations; ++it) {
        if (it < cap_state)
            HV_HIP(hipMemcpyAsync(d_tstate + (size_t)it * 16 * (size_t)N, T, 128 * (size_t)N, hipMemcpyDeviceToDevice, v->stream));
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_pg_linearise, gE, blk, 0, v->stream, (const double *)T, d_nodes, d_Z, d_info, d_unc, (int)E, mu, M21, g,
                           (double *)nullptr, (double *)nullptr, (double *)nullptr, p_F, 0.0, S, 0);
        hipLaunchKernelGGL(k_pg_gather, gN, blk, 0, v->stream, (const int32_t *)d_row, (const int32_t *)d_ent, (const double *)M21, (const double *)g,
                           (int)N, (int)E, fixed, D21, b, p_maxd, p_grad);
        hipLaunchKernelGGL(k_pg_factor, gN, blk, 0, v->stream, S, (const double *)p_maxd, nbN, prm->lambda_scale, (const double *)D21,
                           (const double *)b, (int)N, fixed, L21, x, rr, z, p_rz);
        for (int j = 0; j < prm->cg_max_iterations; ++j) {
            hipLaunchKernelGGL(k_pg_cg_direction, gN, blk, 0, v->stream, S, j, (const double *)p_rz, nbN, tol2, (int)N, (const double *)z, p);
            hipLaunchKernelGGL(k_pg_cg_edges, gE, blk, 0, v->stream, (const PgState *)S, j, d_nodes, (const double *)M21, (int)E, (int)N,
                               (const double *)p, u);
            hipLaunchKernelGGL(k_pg_cg_nodes, gN, blk, 0, v->stream, (const PgState *)S, j, (const int32_t *)d_row, (const int32_t *)d_ent,
                               (const double *)u, (int)N, (int)E, fixed, (const double *)p, qv, p_pq);
            hipLaunchKernelGGL(k_pg_cg_update, gN, blk, 0, v->stream, (const PgState *)S, j, (const double *)p_pq, nbN, (const double *)L21, (int)N,
                               (const double *)p, (const double *)qv, x, rr, z, p_rz);
        }
        hipLaunchKernelGGL(k_pg_trial, gN, blk, 0, v->stream, (const PgState *)S, (const double *)T, (const double *)x, (const double *)b, (int)N, Tn,
                           p_dd, p_pred);
        hipLaunchKernelGGL(k_pg_linearise, gE, blk, 0, v->stream, (const double *)Tn, d_nodes, d_Z, d_info, d_unc, (int)E, mu, (double *)nullptr,
                           (double *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr, p_Fn, 0.0, S, 0);
        hipLaunchKernelGGL(k_pg_decide, dim3(1), dim3(64), 0, v->stream, S, (const double *)p_F, (const double *)p_Fn, nbE, (const double *)p_dd,
                           (const double *)p_pred, (const double *)p_grad, nbN, rules, cap > 0 ? d_trace : (double *)nullptr, cap);
        hipLaunchKernelGGL(k_pg_commit, dim3((unsigned)((n16 + PG_BLOCK - 1) / PG_BLOCK)), blk, 0, v->stream, (const PgState *)S, (const double *)Tn,
                           n16, T);
        hv_profile_end(v, 0);
        HV_HIP(hipGetLastError());
        // the iteration's one host wait
        HV_HIP(hipMemcpyAsync(&hs, S, sizeof(PgState), hipMemcpyDeviceToHost, v->stream));
        HV_HIP(hipStreamSynchronize(v->stream));
        if (hs.stop) break;
    }
    // the final weights at the final state, and the poses to where the caller reads them
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_pg_linearise, gE, blk, 0, v->stream, (const double *)T, d_nodes, d_Z, d_info, d_unc, (int)E, mu, (double *)nullptr,
                       (double *)nullptr, (double *)nullptr, (double *)nullptr, d_w != nullptr ? d_w : d_l, (double *)nullptr,
                       prm->edge_prune_threshold, S, 1);
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    HV_HIP(hipMemcpyAsync(st.dev<double>(i_pout), T, 128 * (size_t)N, hipMemcpyDeviceToDevice, v->stream));
    rc = st.finish(&hs, sizeof(PgState), S);
    if (rc != HV_OK) return rc;
    const int64_t rows = std::min<int64_t>(hs.iter, cap);
    if (rows > 0) {
        HV_HIP(hipMemcpy(trace, d_trace, 8 * HV_POSE_GRAPH_TRACE_STRIDE * (size_t)rows, hipMemcpyDeviceToHost));
        if (cap_state > 0) HV_HIP(hipMemcpy(trace_poses, d_tstate, 128 * (size_t)N * (size_t)rows, hipMemcpyDeviceToHost));
    }
    if (trace_rows) *trace_rows = rows;
    res->chi2_initial = hs.chi2_initial;
    res->chi2_final = hs.chi2_final;
    res->lambda = hs.lambda;
    res->iterations = hs.iter;
    res->cg_iterations_total = hs.cg_total;
    res->edges_kept = hs.kept;
    res->converged = hs.converged;
    res->success = (hs.converged != 0 && hs.bad == 0 && std::isfinite(hs.chi2_final)) ? 1 : 0;
    return HV_OK;
}

extern "C" int hv_pose_graph_linearise(hv_volume *v, const double *poses, int64_t n_nodes, const int32_t *edge_nodes, const double *edge_T,
                                       const double *edge_info, const uint8_t *edge_uncertain, int64_t n_edges, double line_process_weight,
                                       double *r_out, double *chi2_out, double *l_out, double *M_out, double *g_out, double *gradient_out,
                                       int32_t loc) {
    const char *fn = "hv_pose_graph_linearise";
    HV_REQUIRE(v != nullptr && poses != nullptr && edge_nodes != nullptr && edge_T != nullptr && edge_info != nullptr, HV_ERR_INVALID,
               "%s: null argument", fn);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    const int64_t N = n_nodes, E = n_edges;
    HV_REQUIRE(N >= 1 && N <= PG_MAX_NODES && E >= 1 && E <= PG_MAX_EDGES, HV_ERR_INVALID, "%s: bad graph size %lld nodes, %lld edges", fn,
               (long long)N, (long long)E);
    HV_REQUIRE(std::isfinite(line_process_weight) && line_process_weight > 0.0, HV_ERR_INVALID, "%s: line_process_weight must be positive and finite",
               fn);
    HV_HIP(hipSetDevice(v->device));
    PgHostView h;
    int rc = pg_host_view(v, h, poses, N, edge_nodes, edge_T, edge_info, edge_uncertain, E, loc);
    if (rc != HV_OK) return rc;
    rc = pg_check_graph(fn, h.p_poses, N, h.p_nodes, h.p_Z, h.p_info, h.p_unc, E, 0, false);
    if (rc != HV_OK) return rc;
    std::vector<int32_t> csr;
    pg_incidence(h.p_nodes, N, E, csr);
    const int nbE = (int)((E + PG_BLOCK - 1) / PG_BLOCK), nbN = (int)((N + PG_BLOCK - 1) / PG_BLOCK);
    PgLayout lay;
    const size_t o_state = lay.take(sizeof(PgState)), o_csr = lay.take(4 * csr.size());
    const size_t o_M = lay.take(8 * 21 * (size_t)E), o_g = lay.take(8 * 6 * (size_t)E), o_r = lay.take(8 * 6 * (size_t)E);
    const size_t o_chi = lay.take(8 * (size_t)E), o_l = lay.take(8 * (size_t)E);
    const size_t o_D = lay.take(8 * 21 * (size_t)N), o_b = lay.take(8 * 6 * (size_t)N);
    const size_t o_p0 = lay.take(8 * (size_t)nbN), o_p1 = lay.take(8 * (size_t)nbN), o_pF = lay.take(8 * (size_t)nbE);
    rc = hv_ensure_buffer(v, &v->track_buf, &v->track_buf_bytes, lay.off);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->track_buf;
    int32_t *d_row = (int32_t *)(base + o_csr), *d_ent = d_row + N + 1;
    HvStage st(v, loc);
    const int i_pin = st.in(poses, 128 * (size_t)N), i_nodes = st.in(edge_nodes, 8 * (size_t)E), i_Z = st.in(edge_T, 128 * (size_t)E);
    const int i_info = st.in(edge_info, 288 * (size_t)E), i_unc = st.in(edge_uncertain, (size_t)E);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    v->pipe_armed = false;
    HV_HIP(hipMemsetAsync(base + o_state, 0, sizeof(PgState), v->stream));
    HV_HIP(hipMemcpyAsync(d_row, csr.data(), 4 * csr.size(), hipMemcpyHostToDevice, v->stream));
    double *M21 = (double *)(base + o_M), *g = (double *)(base + o_g), *r = (double *)(base + o_r), *chi = (double *)(base + o_chi);
    double *l = (double *)(base + o_l), *D21 = (double *)(base + o_D), *b = (double *)(base + o_b);
    hipLaunchKernelGGL(k_pg_linearise, dim3((unsigned)nbE), dim3(PG_BLOCK), 0, v->stream, st.dev<const double>(i_pin), st.dev<const int32_t>(i_nodes),
                       st.dev<const double>(i_Z), st.dev<const double>(i_info), st.dev<const uint8_t>(i_unc), (int)E, line_process_weight, M21, g, r,
                       chi, l, (double *)(base + o_pF), 0.0, (PgState *)(base + o_state), 0);
    hipLaunchKernelGGL(k_pg_gather, dim3((unsigned)nbN), dim3(PG_BLOCK), 0, v->stream, (const int32_t *)d_row, (const int32_t *)d_ent,
                       (const double *)M21, (const double *)g, (int)N, (int)E, -1, D21, b, (double *)(base + o_p0), (double *)(base + o_p1));
    HV_HIP(hipGetLastError());
    // struct-of-arrays on the device, edge-major rows for the caller (host memory)
    std::vector<double> hM(21 * (size_t)E), hg(6 * (size_t)E), hr(6 * (size_t)E), hb(6 * (size_t)N);
    HV_HIP(hipMemcpyAsync(hM.data(), M21, 8 * hM.size(), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(hg.data(), g, 8 * hg.size(), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(hr.data(), r, 8 * hr.size(), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(hb.data(), b, 8 * hb.size(), hipMemcpyDeviceToHost, v->stream));
    if (chi2_out != nullptr) HV_HIP(hipMemcpyAsync(chi2_out, chi, 8 * (size_t)E, hipMemcpyDeviceToHost, v->stream));
    if (l_out != nullptr) HV_HIP(hipMemcpyAsync(l_out, l, 8 * (size_t)E, hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    for (int64_t e = 0; e < E; ++e) {
        for (int a = 0; a < 6; ++a) {
            if (r_out != nullptr) r_out[e * 6 + a] = hr[(size_t)a * E + e];
            if (g_out != nullptr) g_out[e * 6 + a] = hg[(size_t)a * E + e];
            if (M_out != nullptr)
                for (int c = 0; c < 6; ++c) {
                    const int lo = std::min(a, c), hi = std::max(a, c);
                    M_out[e * 36 + a * 6 + c] = hM[(size_t)(lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)) * E + e];
                }
        }
    }
    if (gradient_out != nullptr)
        for (int64_t i = 0; i < N; ++i)
            for (int a = 0; a < 6; ++a) gradient_out[i * 6 + a] = hb[(size_t)a * N + i];
    return HV_OK;
}
