/* Stand-in for stb_image: no decoder here, every call reports failure (textures stay oracle-only). */
#ifndef MRT_REFSHIM_STB_IMAGE_H
#define MRT_REFSHIM_STB_IMAGE_H
typedef unsigned char stbi_uc;
static inline int stbi_info_from_memory(const stbi_uc*, int, int*, int*, int*) { return 0; }
static inline int stbi_info(const char*, int*, int*, int*) { return 0; }
static inline stbi_uc* stbi_load_from_memory(const stbi_uc*, int, int*, int*, int*, int) { return nullptr; }
static inline stbi_uc* stbi_load(const char*, int*, int*, int*, int) { return nullptr; }
static inline const char* stbi_failure_reason(void) { return "no image decoder in this build"; }
static inline void stbi_image_free(void*) {}
#endif
