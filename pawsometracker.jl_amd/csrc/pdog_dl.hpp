// pdog_dl.hpp — a library opened at run time: "open the first of these names, resolve these symbols, say what failed".
// Plain C++ over <dlfcn.h> (no HIP, no rccl.h): pawsome_group.hip opens RCCL through it, and the host compiler tests it alone
// (tests/group_open_main.cpp), plain and under AddressSanitizer and UBSan.
//
// dlerror() hands out the text of the last failure ONCE: the call that reads it clears it, and a second call returns NULL.
// So it is called once per failed dlopen, and its result is looked at before it is used (a NULL appended to a std::string is
// undefined behaviour — on a machine without the library that was a crash where an error code was due).
#pragma once
#include <dlfcn.h>
#include <string>

namespace pdog {

struct DlLibrary {
    void *handle = nullptr;
    std::string error; // empty: the library is open and every symbol asked for so far was found

    // The first of `names` that dlopen accepts (by SONAME: a copy the process already holds is the one that is used).  None:
    // handle stays null and error = "<what> not found (<the loader's text for the LAST name tried>)".
    template <typename Names>
    void open_first(const char *what, const Names &names)
    {
        std::string reason = "dlopen failed";
        for (const char *name : names) {
            handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (handle) return;
            if (const char *e = dlerror()) reason = e;
        }
        error = std::string(what) + " not found (" + reason + ")";
    }

    // The address of `name`, or null; the FIRST symbol that is missing is the one the error names: "<what> lacks <name>".
    void *symbol(const char *what, const char *name)
    {
        void *p = handle ? dlsym(handle, name) : nullptr;
        if (!p && error.empty()) error = std::string(what) + " lacks " + name;
        return p;
    }
};

} // namespace pdog
