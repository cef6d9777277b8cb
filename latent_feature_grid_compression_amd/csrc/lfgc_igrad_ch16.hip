// input-gradient (INPUT_ONLY) instantiations of the backward data kernel for grid channel stride 16
#include "lfgc_bwd_data.h"
int lfgc_igrad_dispatch_ch16(int MT, const LfgcBwdArgs& a, int waves, int h16, int lds_bytes, int grid_data, hipStream_t stream) {
    switch (MT) {
        case 1: return lfgc_launch_bwd_data_any<16, 1, 2, true>(a, waves, h16, lds_bytes, grid_data, stream);
        case 2: return lfgc_launch_bwd_data_any<16, 2, 2, true>(a, waves, h16, lds_bytes, grid_data, stream);
        case 4: return lfgc_launch_bwd_data_any<16, 4, 2, true>(a, waves, h16, lds_bytes, grid_data, stream);
        default: return LFGC_E_UNSUPPORTED;
    }
}
