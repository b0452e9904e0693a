// Stand-in: everything the reference uses of GLM is in glm/glm.hpp.
#include <glm/glm.hpp>
