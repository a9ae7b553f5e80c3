// kt_prod.hip — kernel instances and their getters (see kernels.hpp).
#include "kernels.hpp"
#include "of3d_k34.hpp"

namespace of3dk {

// K34 instances: W radii with a compiled register ring, wSig 3..7 (others use K3 + K4).  Every
// getter picks by radius and tile height: OF3D_K34_PICK(RW, SA, SB) returns the getter's kernel
// OF3D_K34_KERNEL(RW, S) for radius RW at tile height SA or SB.
#define OF3D_K34_PICK(RW, SA, SB)                                     \
    if (rw == RW) {                                                   \
        if (s == SA) return (const void*)OF3D_K34_KERNEL(RW, SA);     \
        if (s == SB) return (const void*)OF3D_K34_KERNEL(RW, SB);     \
    }

template <typename F, int NP>
const void* k34_fn(int rw, int s, int rb) {
    if (rb == 2) return nullptr;
#define OF3D_K34_KERNEL(RW, S) k_prod_wyx<F, NP, RW, S>
    OF3D_K34_PICK(9, 16, 8)
    OF3D_K34_PICK(12, 16, 8)
    OF3D_K34_PICK(15, 16, 8)
    OF3D_K34_PICK(18, 8, 4)  // register ring of 38-48 rows: shorter tiles
    OF3D_K34_PICK(21, 8, 4)
#undef OF3D_K34_KERNEL
    return nullptr;
}

// Unique-staging instances (k_prod_wyx UQ: no duplicated halo columns, edge replicas copied)
// for 8-wave blocks, cut for 2 waves per SIMD (256 VGPRs: an 8-wave block runs one per CU
// anyway): gradient prefetch 4 rows, phase-B LDS distance 2.  c3 (rw 21): 8-row tiles
// 1.85 ms vs 1.92 (4-row) and 2.02 (duplicate staging, 4-wave blocks); 16-row tiles and
// deeper prefetch (8, 11 rows) or LDS distance 4 within noise.
template <typename F, int NP>
const void* k34_fn_uq(int rw, int s) {
#define OF3D_K34_KERNEL(RW, S) k_prod_wyx<F, NP, RW, S, 4, 2, 4, 2, true>
    OF3D_K34_PICK(21, 8, 4)
    OF3D_K34_PICK(18, 8, 4)
    OF3D_K34_PICK(15, 8, 4)
    OF3D_K34_PICK(12, 8, 4)
    OF3D_K34_PICK(9, 8, 4)
#undef OF3D_K34_KERNEL
    return nullptr;
}

// Wave-specialised instances (k_prod_wyx_ws: npw producer + 16 - npw consumer waves, 64 npw
// staged columns, 128 VGPRs): npw 8 (512 staged columns), and in fp64 npw 9 (576: two blocks
// per 1024-wide row)
// pd: gradient prefetch rows of the producers (2; 4 for fp64 radii up to 15 at 4-row tiles,
// where the 2 rw + 2 row register ring leaves the room)
template <typename F, int NP>
const void* k34_fn_ws(int rw, int s, int npw, int pd) {
    if (npw != 8 && (npw != 9 || sizeof(F) != 8)) return nullptr;
    if (pd == 4) {
        if (sizeof(F) != 8 || s != 4) return nullptr;
#define OF3D_K34_PD4(RW) \
    if (rw == RW) return npw == 8 ? (const void*)k_prod_wyx_ws<F, NP, RW, 4, 4, 2, 8> : (const void*)k_prod_wyx_ws<F, NP, RW, 4, 4, 2, 9>;
        OF3D_K34_PD4(15)
        OF3D_K34_PD4(12)
        OF3D_K34_PD4(9)
#undef OF3D_K34_PD4
        return nullptr;
    }
    if (pd != 2) return nullptr;
#define OF3D_K34_KERNEL(RW, S) \
    (npw == 8 ? (const void*)k_prod_wyx_ws<F, NP, RW, S> : (const void*)k_prod_wyx_ws<F, NP, RW, S, 2, 2, 9>)
    OF3D_K34_PICK(21, 8, 4)
    OF3D_K34_PICK(18, 8, 4)
    OF3D_K34_PICK(15, 8, 4)
    OF3D_K34_PICK(12, 8, 4)
    OF3D_K34_PICK(9, 8, 4)
#undef OF3D_K34_KERNEL
    return nullptr;
}

// Packed-fp32 instances (k_prod_wyx_pk: 4 producer + 4 consumer waves on float2 lanes)
template <int NP>
const void* k34_fn_pk(int rw, int s) {
#define OF3D_K34_KERNEL(RW, S) k_prod_wyx_pk<NP, RW, S>
    OF3D_K34_PICK(21, 8, 4)
    OF3D_K34_PICK(18, 8, 4)
    OF3D_K34_PICK(15, 8, 4)
    OF3D_K34_PICK(12, 8, 4)
    OF3D_K34_PICK(9, 8, 4)
#undef OF3D_K34_KERNEL
    return nullptr;
}
#undef OF3D_K34_PICK

template const void* k34_fn_pk<9>(int, int);
template const void* k34_fn_pk<5>(int, int);

template const void* k34_fn_ws<double, 9>(int, int, int, int);
template const void* k34_fn_ws<double, 5>(int, int, int, int);
template const void* k34_fn_ws<float, 9>(int, int, int, int);
template const void* k34_fn_ws<float, 5>(int, int, int, int);
template const void* k34_fn_uq<double, 9>(int, int);
template const void* k34_fn_uq<double, 5>(int, int);
template const void* k34_fn_uq<float, 9>(int, int);
template const void* k34_fn_uq<float, 5>(int, int);

template const void* k34_fn<double, 9>(int, int, int);
template const void* k34_fn<double, 5>(int, int, int);
template const void* k34_fn<float, 9>(int, int, int);
template const void* k34_fn<float, 5>(int, int, int);

}  // namespace of3dk
