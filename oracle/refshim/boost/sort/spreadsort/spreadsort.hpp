// Stand-in for Boost.Sort's spreadsort header: the one bit cast the reference's BVH names.
#ifndef MRT_REFSHIM_BOOST_SPREADSORT_HPP
#define MRT_REFSHIM_BOOST_SPREADSORT_HPP
#include <cstring>
namespace boost { namespace sort { namespace spreadsort {
template <typename From, typename To>
inline To float_mem_cast(const From& value) {
    static_assert(sizeof(From) == sizeof(To), "same size");
    To out;
    std::memcpy(&out, &value, sizeof(To));
    return out;
}
}}}  // namespace boost::sort::spreadsort
#endif
