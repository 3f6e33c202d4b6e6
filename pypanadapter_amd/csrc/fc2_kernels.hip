// fc2_kernels.hip -- the zoom-2 instantiations of the FC decimator (fc_decim_kernel<2, ...>,
// launch_fc2_decim; path 7): the kernel is fc_kernels.hip's template, compiled
// here as a second translation unit so that the two sets of instantiations build side by side.
#define ZFFT_FC_ZOOM2 1
#include "fc_kernels.hip"
