// curve_bls12_377_msm.hip -- the group-arithmetic kernels of one curve (explicit instantiations; see kernels_msm.hpp)
#include "kernels_bucket.hpp"
#include "kernels_canonical.hpp"
namespace mp {
MP_MSM_KERNELS(template, Bls12_377)
MP_BUCKET_KERNELS(template, Bls12_377)
MP_DECOMPRESS_KERNELS(template, Bls12_377)
MP_CANONICAL_KERNELS(template, Bls12_377)
}
