// Our own stand-in for the one sdsl header that the reference's include/common.hpp pulls in
// (oracle/_ref_drivers/mem_finder_driver.cpp).  It declares only the names common.hpp's
// serialisation templates mention; the match scan never instantiates them, so nothing here
// has to do real work.  No sdsl code is reproduced.
#ifndef MMT_SDSL_SHIM_IO_HPP
#define MMT_SDSL_SHIM_IO_HPP
#include <cstdint>
#include <istream>
#include <ostream>
#include <string>

namespace sdsl {
struct structure_tree_node {};
namespace structure_tree {
inline structure_tree_node* add_child(structure_tree_node*, const std::string&, const std::string&) { return nullptr; }
inline void add_size(structure_tree_node*, uint64_t) {}
}  // namespace structure_tree
namespace util {
template <class T> std::string class_name(const T&) { return "?"; }
}  // namespace util
namespace conf {
constexpr uint64_t SDSL_BLOCK_SIZE = uint64_t(1) << 22;
}  // namespace conf
template <class T> uint64_t serialize(const T& x, std::ostream& out, structure_tree_node* = nullptr, std::string = "") {
    out.write(reinterpret_cast<const char*>(&x), sizeof(x));
    return sizeof(x);
}
template <class T> void load(T& x, std::istream& in) { in.read(reinterpret_cast<char*>(&x), sizeof(x)); }
}  // namespace sdsl
#endif
