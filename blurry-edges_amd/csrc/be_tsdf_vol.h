// The description of a TSDF volume as the kernels of be_tsdf.hip and be_tsdf_mesh.hip take it by value, and its validation.
#pragma once
#include <cstdint>
#include "be_common.h"

namespace be {

// the volume by value: voxel (iz, iy, ix) has its centre at (x0 + ix sx, y0 + iy sy, z0 + iz sz); tensors are [nz,ny,nx], x fastest
struct Vol {
    float x0, y0, z0;
    float sx, sy, sz;
    float trunc;
    int nx, ny, nz;
    int64_t n;
};

inline int make_vol(const char* who, const int* dims, const float* origin, const float* voxel, float trunc, Vol* vol) {
    BE_REQUIRE(dims && origin && voxel, "%s: null pointer", who);
    BE_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && dims[0] <= BE_TSDF_MAX_DIM && dims[1] <= BE_TSDF_MAX_DIM && dims[2] <= BE_TSDF_MAX_DIM,
               "%s: each of dims = (Nz, Ny, Nx) must be in [1, %d], got (%d, %d, %d)", who, BE_TSDF_MAX_DIM, dims[0], dims[1], dims[2]);
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    BE_REQUIRE(n < ((int64_t)1 << 31), "%s: %lld voxels; fewer than 2^31", who, (long long)n);
    const float inf = __builtin_inff();
    for (int a = 0; a < 3; ++a) {
        BE_REQUIRE(origin[a] > -inf && origin[a] < inf, "%s: origin must be finite", who);
        BE_REQUIRE(voxel[a] > 0.0f && voxel[a] < inf, "%s: voxel must be three finite numbers > 0", who);
    }
    BE_REQUIRE(trunc > 0.0f && trunc <= 4.0f, "%s: trunc must be a finite number in (0, 4]", who);
    vol->x0 = origin[0]; vol->y0 = origin[1]; vol->z0 = origin[2];
    vol->sx = voxel[0]; vol->sy = voxel[1]; vol->sz = voxel[2];
    vol->trunc = trunc;
    vol->nz = dims[0]; vol->ny = dims[1]; vol->nx = dims[2];
    vol->n = n;
    return BE_OK;
}

}  // namespace be
