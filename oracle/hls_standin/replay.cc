/*
 * replay.cc -- stand-alone program (its own main) that replays recorded calls of one model's <M>_compute_graphs, so that the
 * reference's sources can run under ASan / UBSan without a sanitizer runtime inside python (make -C oracle ref-replay builds
 * _ref/replay_<model>_<form> from this file, the reference's sources and the stand-in headers; -DENTRY names the entry point).
 * A call file is what tests/ref_pin.py dump_call writes: int32 num_graphs, int32 count, then per array int64 bytes + the bytes,
 * in the entry point's argument order.  Every array is an exact-size heap block, so a read past one is reported.
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

/* every argument after num_graphs is a pointer; the longest list (GCN) has 18 */
extern "C" void ENTRY(int, void*, void*, void*, void*, void*, void*, void*, void*, void*, void*, void*, void*, void*, void*, void*, void*,
                      void*, void*, void*, void*);

int main(int argc, char** argv)
{
    for (int f = 1; f < argc; f++) {
        FILE* fp = std::fopen(argv[f], "rb");
        int num_graphs = 0, count = 0;
        if (!fp || std::fread(&num_graphs, 4, 1, fp) != 1 || std::fread(&count, 4, 1, fp) != 1 || count < 1 || count > 20) {
            std::fprintf(stderr, "replay: cannot read %s\n", argv[f]);
            return 2;
        }
        std::vector<void*> a(20, nullptr);
        for (int i = 0; i < count; i++) {
            long long bytes = 0;
            if (std::fread(&bytes, 8, 1, fp) != 1 || bytes < 0) return 2;
            a[i] = std::malloc(bytes ? (size_t)bytes : 1);
            if (bytes && std::fread(a[i], 1, (size_t)bytes, fp) != (size_t)bytes) return 2;
        }
        std::fclose(fp);
        ENTRY(num_graphs, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15], a[16], a[17],
              a[18], a[19]);
        std::printf("replay ok %s\n", argv[f]);
        for (int i = 0; i < count; i++) std::free(a[i]);
    }
    return 0;
}
