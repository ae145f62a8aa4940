/* stub: mesh_loader.h names objl::Loader; the reference harness loads no meshes */
#ifndef PT_REF_OBJ_LOADER_STUB
#define PT_REF_OBJ_LOADER_STUB
#include <string>
#include <vector>
namespace objl {
struct Vertex {};
struct Mesh { std::vector<Vertex> Vertices; };
struct Loader {
    std::vector<Mesh> LoadedMeshes;
    bool LoadFile(const std::string&) { return false; }
};
}
#endif
