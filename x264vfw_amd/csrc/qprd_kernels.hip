// qprd_kernels.hip — x264gpu_qprd_walk: the QP-RD walk (qprd.hip.h) as a primitive.  One thread per problem runs the state machine of the macroblock
// loop over tables: what an encode at quantiser q would cost (d_cost[p][q]), whether it would code nothing (d_empty[p][q]), and what the encode with the
// other transform size would cost (d_cost_flip[p][q]).  Out come the chosen quantiser, the flip decision and the quantisers asked for, in order.
#include "common.hip.h"
#include "qprd.hip.h"

using namespace x264gpu;

namespace {

__global__ __launch_bounds__(64) void k_qprd_walk(const int32_t *__restrict__ cost, const uint8_t *__restrict__ empty, const int32_t *__restrict__ cost_flip,
                                                  const int32_t *__restrict__ orig_qp, const int32_t *__restrict__ last_qp, const int32_t *__restrict__ t8_eligible,
                                                  int n, int qp_min, int qp_max, int psy, int32_t *__restrict__ out_qp, int32_t *__restrict__ out_flip,
                                                  int32_t *__restrict__ asked, int32_t *__restrict__ n_asked)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const int32_t *ct = cost + (size_t)p * 52, *cf = cost_flip + (size_t)p * 52;
    const uint8_t *et = empty + (size_t)p * 52;
    QprdWalk w;
    int act = qprd_start(w, orig_qp[p], last_qp[p], qp_min, qp_max, psy, t8_eligible[p]), na = 0;
    // (every round asks for one encode and the walk cannot ask for more than two per quantiser and three besides: the bound only fences the output row)
    while (act != QPRD_DONE && na < 2 * 52 + 4) {
        const int q = min(max(w.q, 0), 51);          // (the host admits quantisers 0..51 only; the clamp keeps the lookup inside the row whatever the tables say)
        if (na < X264GPU_QPRD_ASKED_MAX) asked[(size_t)p * X264GPU_QPRD_ASKED_MAX + na] = w.q | (act == QPRD_FLIP ? 256 : 0);
        na++;
        act = qprd_step(w, act == QPRD_FLIP ? cf[q] : ct[q], et[q]);
    }
    out_qp[p] = w.bqp; out_flip[p] = w.flip; n_asked[p] = na;
}

}  // namespace

extern "C" int x264gpu_qprd_walk(const int32_t *d_cost, const uint8_t *d_empty, const int32_t *d_cost_flip, const int32_t *d_orig_qp, const int32_t *d_last_qp,
                                 const int32_t *d_t8_eligible, int n, int qp_min, int qp_max, int psy, int32_t *d_qp, int32_t *d_flip, int32_t *d_asked,
                                 int32_t *d_n_asked, void *stream)
{
    ARG_TRY(n >= 0 && d_cost && d_empty && d_cost_flip && d_orig_qp && d_last_qp && d_t8_eligible && d_qp && d_flip && d_asked && d_n_asked);
    ARG_TRY(qp_min >= 0 && qp_min <= qp_max && qp_max <= 51);
    if (!n) return X264GPU_OK;
    hipLaunchKernelGGL(k_qprd_walk, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_cost, d_empty, d_cost_flip, d_orig_qp, d_last_qp, d_t8_eligible, n,
                       qp_min, qp_max, psy, d_qp, d_flip, d_asked, d_n_asked);
    HIP_TRY(hipGetLastError());
    return X264GPU_OK;
}
