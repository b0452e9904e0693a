// Stand-in for Boost.Assert: the one macro the reference's ASSERT expands to (debug builds only).
#ifndef MRT_REFSHIM_BOOST_ASSERT_HPP
#define MRT_REFSHIM_BOOST_ASSERT_HPP
#include <cassert>
#define BOOST_ASSERT_MSG(condition, message) assert((condition) && (message))
#endif
