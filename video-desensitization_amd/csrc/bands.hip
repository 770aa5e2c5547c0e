// bands.hip — letterbox bands: the publish step behind the stem's and layer1's band tiles
// (BandArgs in vd_common.h, band_tag in vd_kernel.h, the row rule in face_bands.h).
//
// The band ops' kernels only READ the tags: a frame whose tag equals the call's conditions keeps
// its band tiles and takes their maximum from bmax; any other frame runs them and collects their
// maximum in scratch. This kernel runs once per frame group after the group's last op, when every
// workgroup of every band op has decided: it replaces the tags that did not match, stores the
// maxima that go with them, and counts both outcomes for vdt_face_band_stats.
#include "vd_kernel.h"

namespace {

__global__ __launch_bounds__(256) void band_publish_kernel(BandPublishArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 4 * a.n) return;
    const int k = i / a.n, f = i - k * a.n;
    const BandArgs& d = a.op[k];
    if (!d.on) return;
    const unsigned long long cur = band_tag(d, f);
    if (d.tag[f] == cur) {
        atomicAdd(a.stats + 2 * k, 1u);
        return;
    }
    a.tag[k][f] = cur;
    a.bmax[k][f] = d.scratch[f];
    atomicAdd(a.stats + 2 * k + 1, 1u);
}

}  // namespace

hipError_t vd_launch_band_publish(const BandPublishArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(band_publish_kernel, dim3((4 * a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}
