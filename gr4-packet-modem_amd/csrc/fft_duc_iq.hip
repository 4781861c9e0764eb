// fft_duc_iq.hip -- the integer instantiations of the FftDuc's inverse kernel (fft_duc_inverse.hpp)
// and their launch, in a unit of their own: beside them in one unit the complex64 instantiation was scheduled differently.
// Built with fft_duc.hip's flags; iq_format.hpp's pack keeps its product and sum apart under them.
#include "fft_duc_inverse.hpp"

namespace gr4pm {

void fft_duc_launch_inverse_iq(dim3 grid, hipStream_t stream, const InvArgsIq& b, int format)
{
    switch (format) {
    case GR4PM_IQ_SC16: hipLaunchKernelGGL(k_fft_duc_inverse<GR4PM_IQ_SC16>, grid, dim3(kW64Threads), 0, stream, b); break;
    case GR4PM_IQ_SC8: hipLaunchKernelGGL(k_fft_duc_inverse<GR4PM_IQ_SC8>, grid, dim3(kW64Threads), 0, stream, b); break;
    default: hipLaunchKernelGGL(k_fft_duc_inverse<GR4PM_IQ_CU8>, grid, dim3(kW64Threads), 0, stream, b); break;
    }
}

} // namespace gr4pm
