/* stub: the reference harness writes no images; png_image.h only needs the name to exist */
#ifndef PT_REF_STB_WRITE_STUB
#define PT_REF_STB_WRITE_STUB
inline int stbi_write_png(const char*, int, int, int, const void*, int) { return 0; }
#endif
