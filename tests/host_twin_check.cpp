// host_twin_check.cpp -- the library's host twins as a stand-alone program (tests/test_host_twins_sanitized.py): compiled together
// with the seven chroma_amd/csrc/*_host.cpp, plainly and under the address, undefined-behaviour and float-cast-overflow
// sanitizers, it reads ONE call from a file, makes it, and writes the status and every array back raw.  The shared *_common.h
// headers compiled here are the arithmetic the device runs; nothing is loaded into an interpreter and nothing is preloaded.
//
//   host_twin_check CASE OUT
//
// CASE (little-endian, packed; the test writes it from the very arguments it hands the library's twin through ctypes):
//   char[8]  "TWINCALL"
//   u32      length of the twin's name, the name (no terminator)
//   u32      nblobs; per blob: u64 size, `size` bytes.  A blob is an array or a struct of the call as it stood BEFORE the call.
//            Every blob becomes one heap block of exactly its size, so a read or write past an array's end is the sanitizer's.
//   u32      nrelocs; per reloc: u32 blob, u64 offset, u32 target blob, u64 target offset: the pointer-sized word at `offset` of
//            `blob` becomes the address of `target offset` in `target blob` (a struct's pointer members; a null stays the zero
//            word the blob holds).
//   u32      nslots, the call's arguments in order; per slot: u8 kind, then
//              kind 0  u64 bits: an integer (its value, sign-extended to 64 bits) or a float / double (its bits in the low word(s))
//              kind 1  u32 blob, u64 offset: a pointer into a blob
//              kind 2  nothing: a null pointer
// OUT:  i32 status the twin returned, then every blob in order, raw, as it stands AFTER the call (relocated words zeroed again,
//       so the file does not depend on where the heap put things).
// Exit status: 0 when the call was made (whatever it returned), 2 for a bad command line, file or name.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../include/chroma_hip.h"

// the one outside symbol of the twins (context.hip's in the library): the status is what the caller sees
int set_error(int code, const char *fmt, ...)
{
    (void)fmt;
    return code;
}

namespace {

struct Slot { uint64_t bits; void *pointer; };

template <class T> T as(const Slot &s)
{
    if constexpr (std::is_pointer_v<T>) {
        return reinterpret_cast<T>(s.pointer);
    } else if constexpr (std::is_same_v<T, float>) {
        const uint32_t word = (uint32_t)s.bits;
        float f;
        memcpy(&f, &word, sizeof f);
        return f;
    } else if constexpr (std::is_same_v<T, double>) {
        double d;
        memcpy(&d, &s.bits, sizeof d);
        return d;
    } else {
        static_assert(std::is_integral_v<T>, "an argument that is no pointer, float or integer");
        return (T)s.bits;          // (the low bits of the sign-extended value: defined for every integer type)
    }
}

template <class... A, size_t... I> int call(int (*fn)(A...), const std::vector<Slot> &slots, std::index_sequence<I...>)
{
    return fn(as<A>(slots[I])...);
}

template <class... A> int call(int (*fn)(A...), const std::vector<Slot> &slots, bool *ok)
{
    *ok = slots.size() == sizeof...(A);
    return *ok ? call(fn, slots, std::index_sequence_for<A...>{}) : 0;
}

struct Reader {
    FILE *f;
    bool ok = true;
    void bytes(void *to, size_t n) { if (n && fread(to, 1, n, f) != n) ok = false; }
    template <class T> T get() { T v{}; bytes(&v, sizeof v); return v; }
};

struct Reloc { uint32_t blob; uint64_t offset; uint32_t target; uint64_t target_offset; };

int fail(const char *what)
{
    fprintf(stderr, "host_twin_check: %s\n", what);
    return 2;
}

}  // namespace

#define TWIN(name) if (twin == #name) status = call(name, slots, &matched)

int main(int argc, char **argv)
{
    if (argc != 3) return fail("usage: host_twin_check CASE OUT");
    Reader in{fopen(argv[1], "rb")};
    if (!in.f) return fail("cannot open the case");
    char magic[8];
    in.bytes(magic, 8);
    if (!in.ok || memcmp(magic, "TWINCALL", 8)) return fail("not a case file");
    std::string twin(in.get<uint32_t>(), '\0');
    in.bytes(&twin[0], twin.size());
    std::vector<unsigned char *> blobs(in.get<uint32_t>());
    std::vector<uint64_t> sizes(blobs.size());
    for (size_t b = 0; b < blobs.size() && in.ok; b++) {
        sizes[b] = in.get<uint64_t>();
        blobs[b] = (unsigned char *)malloc(sizes[b] ? sizes[b] : 1);
        if (!blobs[b]) return fail("out of memory");
        in.bytes(blobs[b], sizes[b]);
    }
    std::vector<Reloc> relocs(in.ok ? in.get<uint32_t>() : 0);
    for (Reloc &r : relocs) {
        r.blob = in.get<uint32_t>(); r.offset = in.get<uint64_t>(); r.target = in.get<uint32_t>(); r.target_offset = in.get<uint64_t>();
        if (!in.ok || r.blob >= blobs.size() || r.target >= blobs.size() || r.offset + sizeof(void *) > sizes[r.blob] || r.target_offset > sizes[r.target])
            return fail("a relocation outside its blob");
        void *p = blobs[r.target] + r.target_offset;
        memcpy(blobs[r.blob] + r.offset, &p, sizeof p);
    }
    std::vector<Slot> slots(in.ok ? in.get<uint32_t>() : 0);
    for (Slot &s : slots) {
        s.bits = 0; s.pointer = nullptr;
        const uint8_t kind = in.get<uint8_t>();
        if (kind == 0) {
            s.bits = in.get<uint64_t>();
        } else if (kind == 1) {
            const uint32_t b = in.get<uint32_t>();
            const uint64_t offset = in.get<uint64_t>();
            if (!in.ok || b >= blobs.size() || offset > sizes[b]) return fail("an argument outside its blob");
            s.pointer = blobs[b] + offset;
        } else if (kind != 2) {
            return fail("an argument of no kind");
        }
    }
    if (!in.ok) return fail("the case ends early");
    fclose(in.f);

    bool matched = false;
    int status = 0;
    TWIN(chroma_vertex_seed_host);
    TWIN(chroma_direction_seed_host);
    TWIN(chroma_daq_noise_host);
    TWIN(chroma_daq_digitize_host);
    TWIN(chroma_daq_reduce_host);
    TWIN(chroma_steps_count_host);
    TWIN(chroma_steps_generate_host);
    TWIN(chroma_steps_count_media_host);
    TWIN(chroma_steps_generate_media_host);
    TWIN(chroma_particles_advance_host);
    TWIN(chroma_particles_track_host);
    TWIN(chroma_particles_points_host);
    TWIN(chroma_particles_segments_host);
    if (!matched) return fail("no such twin, or not its number of arguments");

    for (const Reloc &r : relocs) memset(blobs[r.blob] + r.offset, 0, sizeof(void *));
    FILE *out = fopen(argv[2], "wb");
    if (!out) return fail("cannot open the output");
    const int32_t status32 = status;
    bool written = fwrite(&status32, sizeof status32, 1, out) == 1;
    for (size_t b = 0; b < blobs.size(); b++) {
        written = written && (sizes[b] == 0 || fwrite(blobs[b], 1, sizes[b], out) == sizes[b]);
        free(blobs[b]);
    }
    if (fclose(out) || !written) return fail("cannot write the output");
    return 0;
}
