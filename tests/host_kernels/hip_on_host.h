// tests/host_kernels/hip_on_host.h -- enough of HIP for g++ to compile the loop-restoration kernel headers as plain C++: the qualifiers
// as empty macros, one lane per workgroup of the tiled kernels (SVTHIP_LR_THREADS = 1: the lane does all of its workgroup's work in order,
// so a barrier is a no-op), blockIdx / threadIdx / blockDim as globals, atomicAdd as a plain add.  launch() walks a grid the way the device
// would, one workgroup and one lane after the other.  Include this first, then the kernel headers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
#define __forceinline__ inline
#define __syncthreads()
#define SVTHIP_LR_THREADS 1

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
static dim3 blockIdx(0, 0, 0), threadIdx(0, 0, 0), blockDim(1, 1, 1);
template <typename T, typename V>
static T atomicAdd(T* p, V v)
{
    const T o = *p;
    *p = (T)(o + (T)v);
    return o;
}
using std::max;
using std::min;

// kernel() once per lane of every workgroup of the grid; kernels whose lanes are independent run with more than one lane per workgroup
template <typename F>
static void launch(dim3 grid, unsigned lanes, F kernel)
{
    blockDim = dim3(lanes);
    for (blockIdx.z = 0; blockIdx.z < grid.z; blockIdx.z++)
        for (blockIdx.y = 0; blockIdx.y < grid.y; blockIdx.y++)
            for (blockIdx.x = 0; blockIdx.x < grid.x; blockIdx.x++)
                for (threadIdx.x = 0; threadIdx.x < lanes; threadIdx.x++) kernel();
    blockIdx = threadIdx = dim3(0, 0, 0);
}

template <typename T>
static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) abort();
    return v;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }
