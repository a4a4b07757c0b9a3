/* The intra kernel's ticket -> cell mapping (svt_intra_cell_of_ticket, csrc/encdec_core.h: the text svt_intra_kernel calls) on the host:
 * for every grid shape given on the command line range, tickets 0 .. rows*cols-1 are a bijection onto the cells, the diagonal never
 * decreases with the ticket, rows ascend inside a diagonal, and the left / above neighbours of every cell hold smaller tickets -- the
 * property that keeps a worker from waiting at a flag nobody sets.  Built and run by tests/test_intra_wavefront.py.
 *     intra_wavefront_check MAX          every (rows, cols) in 1..MAX x 1..MAX, then (135, 240), (240, 135), (1, 512), (512, 1) */
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "encdec_core.h"

static int check_grid(int rows, int cols) {
    const int        n_cell = rows * cols;
    std::vector<int> ticket_of(n_cell, -1);
    int              bad = 0, pd = 0, pr = -1;
    for (int n = 0; n < n_cell; n++) {
        int cr = -1, cc = -1;
        svt_intra_cell_of_ticket(n, rows, cols, &cr, &cc);
        if (cr < 0 || cr >= rows || cc < 0 || cc >= cols) { printf("MISMATCH %dx%d ticket %d: cell (%d, %d) outside the grid\n", rows, cols, n, cr, cc); return 1; }
        int &t = ticket_of[cr * cols + cc];
        if (t >= 0) { printf("MISMATCH %dx%d tickets %d and %d: both cell (%d, %d)\n", rows, cols, t, n, cr, cc); bad++; }
        t = n;
        const int d = cr + cc;
        if (d < pd) { printf("MISMATCH %dx%d ticket %d: diagonal %d after %d\n", rows, cols, n, d, pd); bad++; }
        if (d == pd && cr <= pr) { printf("MISMATCH %dx%d ticket %d: row %d after %d on diagonal %d\n", rows, cols, n, cr, pr, d); bad++; }
        pd = d; pr = cr;
        if (bad > 8) return bad;
    }
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) {
            const int t = ticket_of[r * cols + c];
            if (t < 0) { printf("MISMATCH %dx%d: cell (%d, %d) has no ticket\n", rows, cols, r, c); bad++; continue; }
            if (c > 0 && ticket_of[r * cols + c - 1] >= t) { printf("MISMATCH %dx%d cell (%d, %d): left neighbour's ticket %d >= %d\n", rows, cols, r, c, ticket_of[r * cols + c - 1], t); bad++; }
            if (r > 0 && ticket_of[(r - 1) * cols + c] >= t) { printf("MISMATCH %dx%d cell (%d, %d): above neighbour's ticket %d >= %d\n", rows, cols, r, c, ticket_of[(r - 1) * cols + c], t); bad++; }
            if (bad > 8) return bad;
        }
    return bad;
}

int main(int argc, char **argv) {
    const int max = argc > 1 ? atoi(argv[1]) : 48;
    int       grids = 0, bad = 0;
    for (int r = 1; r <= max; r++)
        for (int c = 1; c <= max; c++) { bad += check_grid(r, c) != 0; grids++; }
    static const int more[4][2] = {{135, 240}, {240, 135}, {1, 512}, {512, 1}};
    for (int k = 0; k < 4; k++) { bad += check_grid(more[k][0], more[k][1]) != 0; grids++; }
    printf("grids %d bad %d\n", grids, bad);
    return bad != 0;
}
