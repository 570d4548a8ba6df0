// BN254 G1 (y^2 = x^3 + 3 over Fq) in extended Jacobian coordinates (X, Y, ZZ, ZZZ): x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2.  The formulas are
// the Explicit-Formulas Database's "xyzz" set for short Weierstrass curves (madd-2008-s, add-2008-s, dbl-2008-s-1 with a = 0).
// Infinity is ZZ = 0 (stored as all zeros); an affine point is infinity when its 64 bytes are zero (ffjavascript's G1.zeroAffine).
// Every exceptional case is decided BY VALUE where it can arise -- nothing assumes distinct or finite operands:
//   accumulator empty            -> the other operand is copied                      (g1_madd, g1_add)
//   other operand infinity       -> accumulator unchanged                            (g1_add; g1_madd's callers drop affine infinity, g1_madd checks again)
//   same x, same y   (P + P)     -> doubling                                         (P == 0 && R == 0)
//   same x, other y  (P + -P)    -> infinity                                         (P == 0 && R != 0)
//   doubling a point with y = 0  -> infinity falls out of the formula (ZZ3 = (2y)^2 ZZ = 0); the coordinates are cleared
// Fq products: madd 8M + 2S, add 12M + 2S, dbl 6M + 3S, to-affine 1 inversion + 5M.
#pragma once
#include "bn_fq.cuh"

namespace bn {

struct G1X { u32 x[8], y[8], zz[8], zzz[8]; };

__device__ __forceinline__ void fq_copy(u32 d[8], const u32 s[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = s[i];
}
__device__ __forceinline__ void g1_set_inf(G1X &p) {
#pragma unroll
    for (int i = 0; i < 8; i++) p.x[i] = p.y[i] = p.zz[i] = p.zzz[i] = 0;
}
__device__ __forceinline__ bool g1_is_inf(const G1X &p) { return fq_is_zero(p.zz); }
__device__ __forceinline__ bool g1_affine_is_inf(const u32 x[8], const u32 y[8]) { return fq_is_zero(x) && fq_is_zero(y); }
__device__ __forceinline__ void g1_neg(G1X &p) { fq_neg(p.y, p.y); }

// p = 2 p
__device__ __forceinline__ void g1_dbl(G1X &p) {
    if (g1_is_inf(p)) return;
    u32 u[8], v[8], w[8], s[8], m[8], t[8];
    fq_dbl(u, p.y);
    fq_sqr(v, u);
    if (fq_is_zero(v)) { g1_set_inf(p); return; }
    fq_mul(w, u, v);
    fq_mul(s, p.x, v);
    fq_sqr(t, p.x); fq_dbl(m, t); fq_add(m, m, t);
    fq_mul(u, w, p.y);                                       // W Y1, before Y is overwritten
    fq_sqr(p.x, m); fq_sub(p.x, p.x, s); fq_sub(p.x, p.x, s);
    fq_sub(t, s, p.x); fq_mul(t, m, t);
    fq_sub(p.y, t, u);
    fq_mul(p.zz, v, p.zz);
    fq_mul(p.zzz, w, p.zzz);
}

// the common end of both additions: from P = U2 - U1, R = S2 - S1 (P != 0), U1, S1 and the product of the operands' ZZ / ZZZ
__device__ __forceinline__ void g1_add_finish(G1X &p, const u32 pd[8], const u32 rd[8], const u32 u1[8], const u32 s1[8]) {
    u32 pp[8], ppp[8], q[8], t[8];
    fq_sqr(pp, pd);
    fq_mul(ppp, pd, pp);
    fq_mul(q, u1, pp);
    fq_mul(t, s1, ppp);                                      // S1 PPP
    fq_sqr(p.x, rd); fq_sub(p.x, p.x, ppp); fq_sub(p.x, p.x, q); fq_sub(p.x, p.x, q);
    fq_sub(q, q, p.x); fq_mul(q, rd, q);
    fq_sub(p.y, q, t);
    fq_mul(p.zz, p.zz, pp);
    fq_mul(p.zzz, p.zzz, ppp);
}

// p += (x, y), an affine point
__device__ __forceinline__ void g1_madd(G1X &p, const u32 x[8], const u32 y[8]) {
    if (g1_affine_is_inf(x, y)) return;
    if (g1_is_inf(p)) {
        fq_copy(p.x, x); fq_copy(p.y, y);
#pragma unroll
        for (int i = 0; i < 8; i++) p.zz[i] = p.zzz[i] = q_one_limb(i);
        return;
    }
    u32 pd[8], rd[8], u1[8], s1[8];
    fq_mul(pd, x, p.zz); fq_sub(pd, pd, p.x);
    fq_mul(rd, y, p.zzz); fq_sub(rd, rd, p.y);
    if (fq_is_zero(pd)) {
        if (fq_is_zero(rd)) g1_dbl(p); else g1_set_inf(p);         // p is the same point as (x, y): double it where it stands
        return;
    }
    fq_copy(u1, p.x); fq_copy(s1, p.y);
    g1_add_finish(p, pd, rd, u1, s1);
}

// p += o
__device__ __forceinline__ void g1_add(G1X &p, const G1X &o) {
    if (g1_is_inf(o)) return;
    if (g1_is_inf(p)) { p = o; return; }
    u32 pd[8], rd[8], u1[8], s1[8];
    fq_mul(u1, p.x, o.zz);
    fq_mul(pd, o.x, p.zz); fq_sub(pd, pd, u1);
    fq_mul(s1, p.y, o.zzz);
    fq_mul(rd, o.y, p.zzz); fq_sub(rd, rd, s1);
    if (fq_is_zero(pd)) {
        if (fq_is_zero(rd)) g1_dbl(p); else g1_set_inf(p);
        return;
    }
    fq_mul(p.zz, p.zz, o.zz);
    fq_mul(p.zzz, p.zzz, o.zzz);
    g1_add_finish(p, pd, rd, u1, s1);
}

// (x, y) = p as an affine point; infinity gives all zeros
__device__ __forceinline__ void g1_to_affine(const G1X &p, u32 x[8], u32 y[8]) {
    if (g1_is_inf(p)) {
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = y[i] = 0;
        return;
    }
    u32 t[8], inv[8];
    fq_mul(t, p.zz, p.zzz);
    fq_inv(inv, t);
    fq_mul(t, inv, p.zzz); fq_mul(x, p.x, t);                // X / ZZ
    fq_mul(t, inv, p.zz); fq_mul(y, p.y, t);                 // Y / ZZZ
}

}  // namespace bn
