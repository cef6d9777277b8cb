// input-gradient (INPUT_ONLY) instantiations of the backward data kernel for grid channel stride 8
#include "lfgc_bwd_data.h"
int lfgc_igrad_dispatch_ch8(int MT, const LfgcBwdArgs& a, int waves, int h16, int lds_bytes, int grid_data, hipStream_t stream) {
    switch (MT) {
        case 1: return lfgc_launch_bwd_data_any<8, 1, 2, true>(a, waves, h16, lds_bytes, grid_data, stream);
        case 2: return lfgc_launch_bwd_data_any<8, 2, 2, true>(a, waves, h16, lds_bytes, grid_data, stream);
        case 4: return lfgc_launch_bwd_data_any<8, 4, 2, true>(a, waves, h16, lds_bytes, grid_data, stream);
        default: return LFGC_E_UNSUPPORTED;
    }
}
