// Prints make_head_geometry of the unmodified csrc/row_tiles.hpp (included below, against the host stand-in for common.hpp), one line
// "vph lph hpb lpr col_blocks tiles grid" per (heads, D, epv, n_rows) of the command line:  emu heads D epv n_rows [heads D epv n_rows ...]
#include "row_tiles.hpp"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    if (argc < 5 || (argc - 1) % 4) return 1;
    for (int i = 1; i + 3 < argc; i += 4) {
        const dgll::rt::HeadGeometry g = dgll::rt::make_head_geometry(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoll(argv[i + 3]));
        printf("%d %d %d %d %d %lld %lld\n", g.vph, g.lph, g.hpb, g.lpr, g.col_blocks, (long long)g.tiles, (long long)g.grid);
    }
    return 0;
}
