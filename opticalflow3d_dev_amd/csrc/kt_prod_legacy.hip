// kt_prod_legacy.hip — kernel instances and their getters (see kernels.hpp).
#include "kernels.hpp"
#include "of3d_k34.hpp"

namespace of3dk {

template <typename F>
const void* k3_kernel(int np, int rw) {
    const int tj = k3_tj(rw);
    if (np == 9)
        return tj == 8 ? (const void*)k_prod_wy<F, 9, 8>
                       : (tj == 12 ? (const void*)k_prod_wy<F, 9, 12> : (const void*)k_prod_wy<F, 9, 24>);
    return tj == 8 ? (const void*)k_prod_wy<F, 5, 8>
                   : (tj == 12 ? (const void*)k_prod_wy<F, 5, 12> : (const void*)k_prod_wy<F, 5, 24>);
}

template <typename F>
const void* k4_kernel(int nf, int rw) {
    const int tj = k4_tj(rw);
    if (nf == 9)
        return tj == 1 ? (const void*)k_wx<F, 9, 1>
                       : (tj == 2 ? (const void*)k_wx<F, 9, 2> : (const void*)k_wx<F, 9, 3>);
    return tj == 1 ? (const void*)k_wx<F, 5, 1> : (tj == 2 ? (const void*)k_wx<F, 5, 2> : (const void*)k_wx<F, 5, 3>);
}

template const void* k3_kernel<double>(int, int);
template const void* k4_kernel<double>(int, int);
template const void* k3_kernel<float>(int, int);
template const void* k4_kernel<float>(int, int);

}  // namespace of3dk
