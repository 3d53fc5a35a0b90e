// rkmh_min_copies.hpp -- the text side of --min-copies, free of everything else so that it can be built on its own
// (tools/asan_bottom): the option's value, and the key a sketch file carries for it.
#pragma once
#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <string>

// a number of 1 .. 2^32 - 1 and nothing else
inline bool min_copies_from_text(const char* text, uint64_t& m) {
    if (!text || !isdigit((unsigned char)*text)) return false;
    char* e = nullptr;
    errno = 0;
    const unsigned long long v = strtoull(text, &e, 10);
    if (errno != 0 || *e != 0 || v < 1 || v > 0xffffffffull) return false;
    m = (uint64_t)v;
    return true;
}
// ,"minCopies":<m> -- in its alphabetical place behind "maxHash" -- for m above 1, else nothing: files made without the option stay
// byte for byte what they were.  The loader finds keys by name and passes over this one.
inline std::string min_copies_json(uint64_t m) { return m > 1 ? ",\"minCopies\":" + std::to_string(m) : std::string(); }
