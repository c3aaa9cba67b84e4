// hk_ocp_soft.hip -- the soft OCP front end's kernels for gfx950: dense problem data of soft-constrained problems
// (the fortran_order_d_ip_ocp_soft_tv wrapper's A, B, b, Q, S, R, q, r, lb, ub, Z, z) -> lib4 stage blocks and the soft
// IPM's constraint vectors in the soft plan's layout, the batched d_res_mpc_soft_tv, and the solver's iterate -> the
// wrapper's outputs with the residual infinity norms.
//
// hk_ocp_soft_pack: hk_ocp_pack's (hk_ocp.hip) two matrix sections with the same element functions (hk_ocp_elem.h):
// one 256-thread workgroup per (section, stage, problem), thread t owns output doubles t, t + 256, .. of the block.
// hk_ocp_soft_pack_vec: one wavefront per (stage, problem), four stages per workgroup.  The stage's vector block is
// [d_k (2 pnb + 2 pns) | Z_k (2 pns) | z_k (2 pns) | ux_k (16, with a warm start) | b row, r / q row (16 each, with
// matrices = 0)]; lane l owns elements l, l + 64, .. of it, decodes which dense element that is and gathers it with
// masked loads (a masked lane reads zero bits; the loads are OR-ed, at most one is live).  The blocks have variable
// length -- pnb + pns reaches 20 doubles per half -- so their places come from the plan's table (oD / oZ).  Every
// element of d_k, Z_k, z_k (and ux_k) is stored, padding as zeros; of the two rows only the live elements are.
//
// hk_ocp_soft_res: d_res_mpc_soft_tv (hk_soft_res, hk_soft.hip) over problem-major arrays, one 256-thread workgroup
// per problem, with that kernel's per-element arithmetic -- a thread per row of r_q / r_b and per constraint of r_d /
// r_z, the inner sums in rising index, the same mu reduction -- so the vectors are those of the one-problem entry
// point.  q is row nu + nx of RSQrq_k; general constraints do not occur (the soft plan refuses them); stage N has no
// inputs, so the reference's "input rows keep the caller's values" never reads `res`.  The reference's quirks are
// hk_soft_res's: soft constraint i of stage k on ux[idxb[k][nu_k + i]] (inside the table only with the plan's
// res_ok), lam_0 - lam_1 on k < N and -lam_2 + lam_3 on k = N, mu over 2 (nb + ns).
//
// hk_ocp_soft_unpack: one wavefront per problem walks the stages; lane l owns variable l of ux, row l of pi and compact
// constraint l of lam / t (2 nb + 4 ns <= 64), and with RES keeps the running maxima of |r_q|, |r_b|, |r_d| over
// exactly the elements the one-problem wrapper visits, from 0; one butterfly reduction at the end.  It is a launch of
// its own, not the residual kernel's epilogue: the finish without norms runs it alone.
#include <hip/hip_runtime.h>

#include "hk_launch.h"
#include "hk_launch_guard.h"
#include "hk_ocp_elem.h"
#include "hk_ocp_soft_args.h"
#include "hk_prims.h"
#include "hpmpc_kargs.h"

namespace {

constexpr int PACK_THREADS = 256;
constexpr int RT = 256;

__device__ __forceinline__ double q4(const double* A, int sd, int i, int j) {
    return A[(i >> 2) * 4 * sd + (i & 3) + 4 * j];
}

}  // namespace

__global__ __launch_bounds__(PACK_THREADS) void hk_ocp_soft_pack(OcpSoftPackArgs a) {
    const unsigned n1 = a.N + 1;
    const int sec = blockIdx.x & 1;  // OCP_SEC_BABT, OCP_SEC_RSQ
    const unsigned sp = blockIdx.x >> 1;
    const int k = sp % n1;
    const unsigned pi = sp / n1;
    if (pi >= (unsigned)a.count) return;
    const long p = (long)a.p0 + pi;
    if (p >= a.nprob) return;
    const OcpStage* sg = &a.st[k].o;
    const OcpStage s = *sg;
    const bool rm = a.row_major != 0;
    // the section's dense arrays are neighbours: A B b | Q S R q r
    const int first = sec == OCP_SEC_BABT ? OCP_A : OCP_Q;
    const int cnt = sec == OCP_SEC_BABT ? 3 : 5;
    const double* P[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const int ai = first + (i < cnt ? i : 0);
        P[i] = a.in[ai].p + p * a.in[ai].s + sg->dn[ai];
    }
    const int n = sg->n[sec], sd = sg->sd[sec];  // n = 0: stage N has no BAbt block
    double* out = (sec == OCP_SEC_BABT ? a.BAbt + p * a.sB : a.RSQ + p * a.sR) + sg->o[sec];
    for (int e = threadIdx.x; e < n; e += PACK_THREADS) {
        int i, j;
        lib4_rc(e, sd, i, j);
        out[e] = sec == OCP_SEC_BABT ? babt_elem(s, P[0], P[1], P[2], rm, i, j)
                                     : rsq_elem(s, P[0], P[1], P[2], P[3], P[4], rm, i, j);
    }
}

__global__ __launch_bounds__(PACK_THREADS) void hk_ocp_soft_pack_vec(OcpSoftPackArgs a) {
    const unsigned groups = (a.N + 4) / 4;
    const unsigned pi = blockIdx.x / groups;
    // the wavefront's stage, as a scalar: the masked loads take wave-uniform bases
    const int k = (blockIdx.x % groups) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (pi >= (unsigned)a.count || k > a.N) return;
    const long p = (long)a.p0 + pi;
    if (p >= a.nprob) return;
    const OcpSoftStage s = a.st[k];
    const OcpStage& o = s.o;
    const int l = threadIdx.x & 63;
    const int nu = o.nu, nux = o.nu + o.nx, nb = o.nb, pnb = o.pnb, ns = s.ns, pns = s.pns;
    const int nd = 2 * pnb + 2 * pns, nz = 2 * pns;
    const int eZ = nd, ez = eZ + nz, eW = ez + nz, eR = eW + (a.ux ? V16 : 0), total = eR + (a.matrices ? 0 : 2 * V16);
    const auto in = [&](int i) { return a.in[i].p + p * a.in[i].s; };
    const double *lb = in(OCP_lb), *ub = in(OCP_ub), *Zi = in(OCPS_Z), *zi = in(OCPS_z), *bi = in(OCP_b),
                 *ri = in(OCP_r), *qi = in(OCP_q);
    const bool hz = a.in[OCPS_z].p != nullptr, hw = a.ux != nullptr;
    const double *u0 = hw ? a.u0 + p * a.su : nullptr, *x0 = hw ? a.x0 + p * a.sx : nullptr;
    for (int e = l; e < total; e += 64) {
        // d_k = [lb pnb | ub pnb | ls pns | us pns], the soft bounds at lb / ub [nb + i]
        const int c1 = e - pnb, c2 = e - 2 * pnb, c3 = c2 - pns;
        // Z_k / z_k = [lower pns | upper pns] from [lower ns | upper ns]
        const int cZ = e - eZ, cz = e - ez;
        const int hZ = cZ >= pns ? 1 : 0, iZ = cZ - hZ * pns, hzz = cz >= pns ? 1 : 0, iz = cz - hzz * pns;
        // ux_k = [u0_k | x0_k | 0 ..]; the rows: b_k, then [r_k | q_k]
        const int cw = e - eW, cr = e - eR, cq = cr - V16;
        const double w[11] = {
            hk::gld(lb, o.dn[OCP_lb] + e, e < nb),
            hk::gld(ub, o.dn[OCP_ub] + c1, c1 >= 0 && c1 < nb),
            hk::gld(lb, o.dn[OCP_lb] + nb + c2, c2 >= 0 && c2 < ns),
            hk::gld(ub, o.dn[OCP_ub] + nb + c3, c3 >= 0 && c3 < ns),
            hk::gld(Zi, s.dnZ + hZ * ns + iZ, cZ >= 0 && cZ < nz && iZ < ns),
            hk::gld(zi, s.dnZ + hzz * ns + iz, hz && cz >= 0 && cz < nz && iz < ns),
            hk::gld(u0, o.dn[OCP_r] + cw, hw && cw >= 0 && cw < nu && e < eR),
            hk::gld(x0, o.dn[OCP_q] + (cw - nu), hw && cw >= nu && cw < nux && e < eR),
            hk::gld(bi, o.dn[OCP_b] + cr, cr >= 0 && cr < o.nx1),
            hk::gld(ri, o.dn[OCP_r] + cq, cq >= 0 && cq < nu),
            hk::gld(qi, o.dn[OCP_q] + (cq - nu), cq >= nu && cq < nux)};
        long long bits = 0;
#pragma unroll
        for (int i = 0; i < 11; i++) bits |= __double_as_longlong(w[i]);
        const double v = __longlong_as_double(bits);
        if (e < eZ)
            a.d[p * a.sD + s.oD + e] = v;
        else if (e < ez)
            a.Z[p * a.sZ + s.oZ + cZ] = v;
        else if (e < eW)
            a.z[p * a.sZ + s.oZ + cz] = v;
        else if (e < eR)
            a.ux[p * a.sV16 + k * V16 + cw] = v;
        else if (cr < V16) {
            if (o.n[OCP_SEC_BABT] > 0 && cr < o.nx1)
                a.BAbt[p * a.sB + o.o[OCP_SEC_BABT] + lib4_at(o.sd[OCP_SEC_BABT], nux, cr)] = v;
        } else if (cq < nux) {
            a.RSQ[p * a.sR + o.o[OCP_SEC_RSQ] + lib4_at(o.sd[OCP_SEC_RSQ], nux, cq)] = v;
        }
    }
}

__global__ __launch_bounds__(RT) void hk_ocp_soft_res(OcpSoftResArgs a) {
    __shared__ double red[RT];
    if (blockIdx.x >= (unsigned)a.count) return;
    const long p = (long)a.p0 + blockIdx.x;
    if (p >= a.nprob) return;
    const int tid = threadIdx.x;
    const long n1 = a.N + 1;
    const double *BAbt = a.BAbt + p * a.sB, *RSQ = a.RSQ + p * a.sR, *D = a.d + p * a.sD, *Zp = a.Z + p * a.sZ,
                 *zp = a.z + p * a.sZ, *UX = a.ux + p * a.sV16, *PI = a.pi + p * a.sV16, *LAM = a.lam + p * a.sC,
                 *T = a.t + p * a.sC;
    double* RQ = a.res + p * a.sRes;
    double* RB = RQ + n1 * V16;
    double* RD = RB + n1 * V16;
    double* RZ = RD + a.sD;
    double musum = 0.0;
    long ntot = 0;
    for (int k = 0; k <= a.N; k++) {
        const OcpSoftStage s = a.st[k];
        const int nu = s.o.nu, nux = s.o.nu + s.o.nx, nb = s.o.nb, pnb = s.o.pnb, ns = s.ns, pns = s.pns,
                  nx1 = s.o.nx1, os = 2 * s.o.pnb, sdQ = s.o.sd[OCP_SEC_RSQ], sdB = s.o.sd[OCP_SEC_BABT];
        const bool last = k == a.N;
        const int* ib = a.idxb + k * 16;
        const double *ux = UX + k * V16, *lam = LAM + s.oC, *t = T + s.oC, *d = D + s.oD;
        const double* Q = RSQ + s.o.o[OCP_SEC_RSQ];
        ntot += nb + ns;
        // mu partial sums
        for (int j = tid; j < nb; j += RT) musum += lam[j] * t[j] + lam[pnb + j] * t[pnb + j];
        for (int j = tid; j < ns; j += RT)
            musum += lam[os + j] * t[os + j] + lam[os + pns + j] * t[os + pns + j] + lam[os + 2 * pns + j] * t[os + 2 * pns + j] +
                     lam[os + 3 * pns + j] * t[os + 3 * pns + j];
        // r_d (negated) and r_z
        double* rd = RD + s.oD;
        for (int j = tid; j < nb; j += RT) {
            const double x = ux[ib[j]];
            rd[j] = -(x - d[j] - t[j]);
            rd[pnb + j] = -(-x + d[pnb + j] - t[pnb + j]);
        }
        for (int j = tid; j < ns; j += RT) {
            const double x = ux[ib[nu + j]];
            rd[os + j] = -(t[os + 2 * pns + j] + x - d[os + j] - t[os + j]);
            rd[os + pns + j] = -(t[os + 3 * pns + j] - x + d[os + pns + j] - t[os + pns + j]);
            const double *Z = Zp + s.oZ, *z = zp + s.oZ;
            double* rz = RZ + s.oZ;
            rz[j] = z[j] + Z[j] * t[os + 2 * pns + j] - lam[os + j] - lam[os + 2 * pns + j];
            rz[pns + j] = z[pns + j] + Z[pns + j] * t[os + 3 * pns + j] - lam[os + pns + j] - lam[os + 3 * pns + j];
        }
        // r_q (negated): row i by one thread; q_k is row nux of RSQrq_k
        double* rq = RQ + k * V16;
        const int nsym = last ? s.o.nx : nux;
        for (int i = tid; i < nux; i += RT) {
            double v;
            if (i < nu)
                v = -q4(Q, sdQ, nux, i);
            else
                v = -q4(Q, sdQ, nux, i) + (k > 0 ? PI[(k - 1) * V16 + i - nu] : 0.0);
            if (i < nsym) {
                double acc = 0.0;
                for (int j = 0; j < nsym; j++) acc += (i >= j ? q4(Q, sdQ, i, j) : q4(Q, sdQ, j, i)) * ux[j];
                v -= acc;
            }
            for (int j = 0; j < nb; j++)
                if (ib[j] == i) v += lam[j] - lam[pnb + j];
            for (int j = 0; j < ns; j++)
                if (ib[nu + j] == i)
                    v += last ? -lam[os + 2 * pns + j] + lam[os + 3 * pns + j] : lam[os + j] - lam[os + pns + j];
            if (!last) {
                const double* Bt = BAbt + s.o.o[OCP_SEC_BABT];
                const double* pi = PI + k * V16;
                double acc = 0.0;
                for (int j = 0; j < nx1; j++) acc += q4(Bt, sdB, i, j) * pi[j];
                v -= acc;
            }
            rq[i] = -v;
        }
        // r_b (negated): x_{k+1} - A x - B u - b
        if (!last) {
            const double* Bt = BAbt + s.o.o[OCP_SEC_BABT];
            const double* ux1 = UX + (k + 1) * V16;
            const int nu1 = a.st[k + 1].o.nu;
            double* rb = RB + k * V16;
            for (int j = tid; j < nx1; j += RT) {
                double acc = 0.0;
                for (int i = 0; i < nux; i++) acc += q4(Bt, sdB, i, j) * ux[i];
                rb[j] = -(ux1[nu1 + j] - q4(Bt, sdB, nux, j) - acc);
            }
        }
    }
    red[tid] = musum;
    __syncthreads();
    for (int w = RT / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) a.mu[p] = ntot != 0 ? red[0] / (2.0 * ntot) : 0.0;
}

// RES: the residual maxima and mu go to a.inf.
template <bool RES>
__global__ __launch_bounds__(64) void hk_ocp_soft_unpack(OcpSoftUnpackArgs a) {
    if (blockIdx.x >= (unsigned)a.count) return;
    const long p = (long)a.p0 + blockIdx.x;
    if (p >= a.nprob) return;
    const int l = threadIdx.x;
    const long n1 = a.N + 1;
    const double *ux = a.ux + p * a.sV16, *pi = a.pi + p * a.sV16, *lam = a.lam + p * a.sC, *t = a.t + p * a.sC;
    const double *rq = nullptr, *rb = nullptr, *rd = nullptr;
    if constexpr (RES) {
        rq = a.res + p * a.sRes;
        rb = rq + n1 * V16;
        rd = rb + n1 * V16;
    }
    double* u = a.out.u + p * a.out.su;
    double* x = a.out.x + p * a.out.sx;
    double* po = a.out.pi + p * a.out.sp;
    double* lo = a.out.lam + p * a.out.sl;
    double* to = a.out.t ? a.out.t + p * a.out.sl : nullptr;
    double mq = 0.0, mb = 0.0, md = 0.0;
    for (int k = 0; k <= a.N; k++) {
        const OcpSoftStage s = a.st[k];
        const int nu = s.o.nu, nux = s.o.nu + s.o.nx, nb = s.o.nb, pnb = s.o.pnb, ns = s.ns, pns = s.pns;
        const bool hv = l < nux, hp = l < s.o.nx1, hc = l < 2 * nb + 4 * ns;
        // compact element l of [lo nb | up nb | 4 x ns] sits at slot src of [lo pnb | up pnb | 4 x pns]
        const int m = l - 2 * nb, blk = m / (ns > 0 ? ns : 1);
        const int src = s.oC + (l < nb ? l : l < 2 * nb ? pnb + (l - nb) : 2 * pnb + blk * pns + (m - blk * ns));
        const double vux = hk::gld(ux, k * V16 + l, hv), vpi = hk::gld(pi, k * V16 + l, hp),
                     vlam = hk::gld(lam, src, hc), vt = hk::gld(t, src, hc && to);
        if (l < nu)
            u[s.o.dn[OCP_r] + l] = vux;
        else if (hv)
            x[s.o.dn[OCP_q] + (l - nu)] = vux;
        if (hp) po[s.o.dn[OCP_b] + l] = vpi;
        if (hc) {
            lo[s.olam + l] = vlam;
            if (to) to[s.olam + l] = vt;
        }
        if constexpr (RES) {
            const bool hb = l < nb, hs = l < ns;
            const int od = s.oD + l;
            mq = fmax(mq, fabs(hk::gld(rq, k * V16 + l, hv)));
            mb = fmax(mb, fabs(hk::gld(rb, k * V16 + l, hp)));
            md = fmax(md, fmax(fabs(hk::gld(rd, od, hb)), fabs(hk::gld(rd, od + pnb, hb))));
            md = fmax(md, fmax(fabs(hk::gld(rd, od + 2 * pnb, hs)), fabs(hk::gld(rd, od + 2 * pnb + pns, hs))));
        }
    }
    if constexpr (RES) {
        mq = wave_max(mq);
        mb = wave_max(mb);
        md = wave_max(md);
        if (l == 0) {
            double* inf = a.inf + 4 * p;
            inf[0] = mq;
            inf[1] = mb;
            inf[2] = md;
            inf[3] = a.mu[p];
        }
    }
}

// matrices != 0: the two matrix sections, then the vectors; else the vectors with the b and r / q rows
extern "C" int hk_ocp_soft_pack_launch(const OcpSoftPackArgs* a, hipStream_t stream) {
    if (a->count <= 0) return 0;
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_ocp_soft_pack));
    static const HkKernelLimits lim_vec(reinterpret_cast<const void*>(&hk_ocp_soft_pack_vec));
    if (const int e = lim.check(0, PACK_THREADS)) return e;
    if (const int e = lim_vec.check(0, PACK_THREADS)) return e;
    const long long blocks = (long long)a->count * (a->N + 1) * 2, vblocks = (long long)a->count * ((a->N + 4) / 4);
    if (blocks > 0x7fffffffLL) return HK_LAUNCH_REFUSED;
    if (a->matrices) {
        hipLaunchKernelGGL(hk_ocp_soft_pack, dim3((unsigned)blocks), dim3(PACK_THREADS), 0, stream, *a);
        if (const int e = (int)hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(hk_ocp_soft_pack_vec, dim3((unsigned)vblocks), dim3(PACK_THREADS), 0, stream, *a);
    return (int)hipGetLastError();
}

extern "C" int hk_ocp_soft_res_launch(const OcpSoftResArgs* a, hipStream_t stream) {
    if (a->count <= 0) return 0;
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_ocp_soft_res));
    if (const int e = lim.check(0, RT)) return e;
    hipLaunchKernelGGL(hk_ocp_soft_res, dim3((unsigned)a->count), dim3(RT), 0, stream, *a);
    return (int)hipGetLastError();
}

// a->res set: with the residual maxima
extern "C" int hk_ocp_soft_unpack_launch(const OcpSoftUnpackArgs* a, hipStream_t stream) {
    if (a->count <= 0) return 0;
    const auto kernel = a->res ? &hk_ocp_soft_unpack<true> : &hk_ocp_soft_unpack<false>;
    static const HkKernelLimits lim[2] = {HkKernelLimits(reinterpret_cast<const void*>(&hk_ocp_soft_unpack<false>)),
                                          HkKernelLimits(reinterpret_cast<const void*>(&hk_ocp_soft_unpack<true>))};
    if (const int e = lim[a->res ? 1 : 0].check(0, 64)) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)a->count), dim3(64), 0, stream, *a);
    return (int)hipGetLastError();
}
