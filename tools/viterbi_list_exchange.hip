// viterbi_list_exchange.hip -- both forms of the list decoder's metric exchange behind one call, for tools/ecc_list_bench.py: the kernel of
// csrc/gswm_viterbi_list.inc instantiated with the predecessors' metrics fetched through the wave's LDS buffer (lds_exchange = 1) and with 2 L ds_bpermute
// (lds_exchange = 0), at every list size.  The library ships one form per list size (viterbi_list::lds_exchange<L>); this file exists so that the choice can
// be measured again.  Built by the tool into tools/build/libvlx.so; not part of libgswm.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>

#include "../include/gswm.h"

__attribute__((visibility("hidden"))) thread_local int g_last_hip_error = 0;   // declared in gswm_host.h

#include "../a-watermark-for-diffusion-models_amd/csrc/gswm_host.h"
#include "../a-watermark-for-diffusion-models_amd/csrc/gswm_viterbi_plan.h"
#include "../a-watermark-for-diffusion-models_amd/csrc/gswm_viterbi_list_plan.h"
#include "../a-watermark-for-diffusion-models_amd/csrc/gswm_viterbi_rate_plan.h"
#include "../a-watermark-for-diffusion-models_amd/csrc/gswm_viterbi.inc"
#include "../a-watermark-for-diffusion-models_amd/csrc/gswm_viterbi_list.inc"

namespace {

template <int L, bool LDSX>
int launch_as(const ViterbiListPlan& p, const viterbi_list::ListArgs& a, hipStream_t stream) {
    const void* k = (const void*)viterbi_list::gsw_viterbi_list_kernel<L, LDSX>;
    GSW_HIP(allow_dynamic_lds(k, p.lds));
    hipLaunchKernelGGL((viterbi_list::gsw_viterbi_list_kernel<L, LDSX>), dim3((uint32_t)p.grid), dim3((uint32_t)p.wg), p.lds, stream, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

template <int L>
int launch_either(int lds_exchange, const ViterbiListPlan& p, const viterbi_list::ListArgs& a, hipStream_t stream) {
    return lds_exchange ? launch_as<L, true>(p, a, stream) : launch_as<L, false>(p, a, stream);
}

}  // namespace

// gsw_viterbi_list_decode's arguments after the exchange to use; the same plan, the same refusals
extern "C" __attribute__((visibility("default"))) int vlx_decode(int lds_exchange, const int32_t* score_dev, int64_t score_stride, int B, int message_bits,
                                                                  int list_size, uint8_t* info_dev, uint8_t* message_dev, int32_t* metric_dev,
                                                                  int32_t* flips_dev, int32_t* ok_dev, int32_t* rank_dev, int32_t* n_ok_dev, void* stream) {
    ViterbiListQuery q{};
    q.pointers_ok = score_dev && info_dev && message_dev && metric_dev && flips_dev && ok_dev && rank_dev && n_ok_dev;
    q.B = B;
    q.L = list_size;
    q.M = message_bits;
    q.stride = score_stride;
    const ViterbiListPlan p = viterbi_list_decide(q);
    if (p.status != GSW_OK) return p.status;
    const viterbi_list::ListArgs a{score_dev, info_dev, message_dev, metric_dev, flips_dev, ok_dev, rank_dev, n_ok_dev, score_stride, B, p.M, p.T, p.I,
                                   p.info_bytes, p.payload_bytes, p.S, p.Sinv, p.full_from, p.wave_lds, p.M};
    switch (p.L) {
        case 1: return launch_either<1>(lds_exchange, p, a, (hipStream_t)stream);
        case 2: return launch_either<2>(lds_exchange, p, a, (hipStream_t)stream);
        case 4: return launch_either<4>(lds_exchange, p, a, (hipStream_t)stream);
        default: return launch_either<8>(lds_exchange, p, a, (hipStream_t)stream);
    }
}

// which form the library ships for a list size
extern "C" __attribute__((visibility("default"))) int vlx_shipped(int list_size) {
    switch (list_size) {
        case 1: return viterbi_list::lds_exchange<1>();
        case 2: return viterbi_list::lds_exchange<2>();
        case 4: return viterbi_list::lds_exchange<4>();
        default: return viterbi_list::lds_exchange<8>();
    }
}
