// capi_staged_out.hpp -- outputs that may live on the host, declared ONCE: from one declaration per output come the bytes its
// workspace slice adds to the caller's size, the device pointer the kernels write to, and (staged_copy_back, capi_keyed_frame.hpp)
// the copy back to the caller.  Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency
// order).  Plain C++ without HIP types: tests/staged_out_check.cpp compiles this file alone with a host compiler.
#pragma once

// slices of a workspace block in order, each rounded up to 256 bytes.  No bounds check: the block must hold what is taken.
struct Bump {
    char* p;
    static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
    template <typename U>
    U* take(size_t count) {
        char* r = p;
        p += up(count * sizeof(U));
        return reinterpret_cast<U*>(r);
    }
    void* operator()(size_t bytes) { return take<char>(bytes); }  // (the allocator form StagedOuts::place takes)
};

// The outputs of one unit class of an entry point: `cap` units (groups or rows) of room each, `host`: the caller's buffers are host
// memory.  An output is STAGED when the kernels cannot write to the caller's buffer: they then write to a workspace slice, which
// staged_copy_back sends to the caller if the caller is on the host and gave a buffer.
struct StagedOuts {
    enum Kind {
        kOut,      // staged on a host frame; a null output is absent: no bytes, a null device pointer
        kOutRoom,  // kOut, but a host frame counts the bytes of an absent output too (a workspace size that does not depend on which
                   // optional outputs a call asks for)
        kScratch   // staged on a host frame AND when the caller gave none: the kernels need it either way; never copied back then
    };
    static constexpr int kMax = 12;  // (the grouped report's 9 are the most)
    struct Out {
        void* user;         // the caller's buffer (nullable)
        void* dev_at;       // where the caller keeps the device pointer (a U* variable)
        size_t unit_bytes;  // bytes per unit
        size_t room;        // bytes of the workspace counted for it
        bool staged, back;
    };
    Out outs[kMax];
    int n = 0;
    size_t cap;
    bool host, stage;

    // stage_on_device: stage the kOut / kOutRoom outputs of a DEVICE frame as well (results that are rearranged before they reach the caller)
    StagedOuts(bool host_space, size_t cap_units, bool stage_on_device = false) : cap(cap_units), host(host_space), stage(host_space || stage_on_device) {}

    // *dev is set to `user` at once: an output that is not staged is written where the caller wants it
    template <typename U>
    void add(U** dev, U* user, size_t per_unit, Kind kind = kOut) {
        if (n == kMax) std::abort();  // (a declaration too many: seen by the first call of the entry point that makes it)
        Out& o = outs[n++];
        o.user = user;
        o.dev_at = dev;
        o.unit_bytes = per_unit * sizeof(U);
        o.staged = kind == kScratch ? (stage || !user) : (stage && user);
        o.room = (o.staged || (kind == kOutRoom && stage)) ? Bump::up(cap * o.unit_bytes) : 0;
        o.back = host && o.staged && user;
        *dev = user;
    }

    // what the slices add to the caller's workspace size: Bump::up per slice, 0 when nothing is staged
    size_t bytes() const {
        size_t b = 0;
        for (int i = 0; i < n; ++i) b += outs[i].room;
        return b;
    }

    // the staged outputs' slices from take(bytes) -> void* (a Bump, or a lambda over ws_take), in declaration order
    template <typename Take>
    void place(Take&& take) {
        for (int i = 0; i < n; ++i) {
            if (!outs[i].staged) continue;
            void* d = take(cap * outs[i].unit_bytes);
            std::memcpy(outs[i].dev_at, &d, sizeof(void*));
        }
    }

    void* dev(int i) const {
        void* d;
        std::memcpy(&d, outs[i].dev_at, sizeof(void*));
        return d;
    }
};
