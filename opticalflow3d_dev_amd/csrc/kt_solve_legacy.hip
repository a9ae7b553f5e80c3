// kt_solve_legacy.hip — kernel instances and their getters (see kernels.hpp).
#include "kernels.hpp"
#include "of3d_k5.hpp"

namespace of3dk {

template <typename F, typename RelT>
const void* k5_kernel(int rw) {
    const int nj = k5_nj(rw);
    if (k5_geom(rw).r == 8)
        return nj == 12 ? (const void*)k_wz_solve<F, RelT, 12, 8, 8> : (const void*)k_wz_solve<F, RelT, 14, 8, 8>;
    switch (nj) {
        case 10: return (const void*)k_wz_solve<F, RelT, 10, 4, 8>;
        case 12: return (const void*)k_wz_solve<F, RelT, 12, 4, 8>;
        default: return (const void*)k_wz_solve<F, RelT, 16, 4, 8>;
    }
}

template <typename F, typename RelT>
const void* k5_dma_kernel(int rw, int nb) {
    const int r = k5_geom(rw).r, nj2 = k5_dma_nj2<F>(rw);
#define OF3D_K5D(NJ2, R)                                                     \
    (nb == 3 ? (const void*)k_wz_solve_dma<F, RelT, NJ2, R, 8, 3>            \
             : (const void*)k_wz_solve_dma<F, RelT, NJ2, R, 8, 2>)
    if constexpr (sizeof(F) == 8) {
        if (r == 8) return nj2 == 6 ? OF3D_K5D(6, 8) : OF3D_K5D(7, 8);
        return nj2 == 6 ? OF3D_K5D(6, 4) : (nj2 == 7 ? OF3D_K5D(7, 4) : OF3D_K5D(8, 4));
    } else {
        if (r == 8) return nj2 == 3 ? OF3D_K5D(3, 8) : OF3D_K5D(4, 8);
        return nj2 == 3 ? OF3D_K5D(3, 4) : OF3D_K5D(4, 4);
    }
#undef OF3D_K5D
}

template const void* k5_kernel<double, float>(int);
template const void* k5_kernel<double, double>(int);
template const void* k5_dma_kernel<double, float>(int, int);
template const void* k5_dma_kernel<double, double>(int, int);
template const void* k5_kernel<float, float>(int);
template const void* k5_kernel<float, double>(int);
template const void* k5_dma_kernel<float, float>(int, int);
template const void* k5_dma_kernel<float, double>(int, int);

}  // namespace of3dk
