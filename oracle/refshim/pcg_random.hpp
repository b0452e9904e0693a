// Stand-in for pcg-cpp: the names the reference's headers mention.  It only has to compile: the two
// PCG samplers are left out of the build and nothing draws from this generator.
#ifndef MRT_REFSHIM_PCG_RANDOM_HPP
#define MRT_REFSHIM_PCG_RANDOM_HPP
#include <random>
namespace pcg_extras {
template <typename RngType>
struct seed_seq_from {};
}  // namespace pcg_extras
struct pcg32 : std::minstd_rand {
    pcg32() = default;
    template <typename SeedSeq>
    explicit pcg32(SeedSeq&) {}
};
#endif
