// Prints the launch geometries of the unmodified csrc/row_tiles.hpp (included below, against the host stand-in for common.hpp):
//   emu heads D epv n_rows [heads D epv n_rows ...]   make_head_geometry, one line "vph lph hpb lpr col_blocks tiles grid" per case
//   emu flat vpr n_rows [vpr n_rows ...]              make_flat_geometry, one line "lpr col_blocks tiles grid" per case
#include "row_tiles.hpp"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "flat")) {
        if (argc < 4 || (argc - 2) % 2) return 1;
        for (int i = 2; i + 1 < argc; i += 2) {
            const dgll::rt::HeadGeometry g = dgll::rt::make_flat_geometry(atoll(argv[i]), atoll(argv[i + 1]));
            printf("%d %d %lld %lld\n", g.lpr, g.col_blocks, (long long)g.tiles, (long long)g.grid);
        }
        return 0;
    }
    if (argc < 5 || (argc - 1) % 4) return 1;
    for (int i = 1; i + 3 < argc; i += 4) {
        const dgll::rt::HeadGeometry g = dgll::rt::make_head_geometry(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoll(argv[i + 3]));
        printf("%d %d %d %d %d %lld %lld\n", g.vph, g.lph, g.hpb, g.lpr, g.col_blocks, (long long)g.tiles, (long long)g.grid);
    }
    return 0;
}
