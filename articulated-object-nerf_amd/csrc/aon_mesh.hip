// Marching cubes on an fp32 grid (mesh extraction from a trained field, aon_marching_cubes): three launches, no atomics, the same bits on
// every run.
//
// Convention (tests/_mc_ref.py is an independent numpy copy):
//   * grid point (i, j, k) has linear index g = (i ny + j) nz + k and position x_a = lo_a + idx_a step_a (multiply, then add, each rounded);
//   * a point is INSIDE iff value > level (NaN is outside);
//   * every point owns its +x, +y, +z edges, and an edge carries a vertex iff exactly one endpoint is inside.  Vertices are ordered by
//     (owning point's g, axis x < y < z), so a vertex id is  [exclusive prefix of vertex counts up to the owner] + [owned lower-axis bits];
//   * the vertex sits at x0 + t (x1 - x0) along the edge, t = (level - v0) / (v1 - v0), every operation rounded (no FMA); when one
//     endpoint is NaN it sits on the other, inside, endpoint;
//   * a cell is named by its lowest corner; its triangles come from the classic 256-case table (corner and edge numbering of Bourke's
//     "Polygonising a scalar field"; the case index has bit c set when corner c is inside), wound so that normals point from high values
//     to low -- outward for a density.  Faces are ordered by (cell's g, triangle order in the table row).
//
// Launches, over tiles of kTile = 1024 consecutive points (256 threads x 4 consecutive points):
//   (a) classify: per point its 3 owned-edge bits and, when it names a cell, the cell's case (one 16-bit word), and its vertex offset
//       inside the tile (16 bits: at most 3 x 1024); per tile the vertex and triangle counts;
//   (b) scan: ONE workgroup turns the per-tile counts into int64 exclusive offsets and the totals V, F (fixed order: the same result on
//       every run without atomics);
//   (c) emit: vertices of the owned edges, and the faces of each cell -- a face's 12 local edges map to vertex ids through the owners'
//       tile offsets, in-tile offsets and lower-axis bits; no per-edge index array exists.
// The eight corner reads of a cell go through the L1 / L2 caches (each value is read by up to 8 cells of the same and the neighbouring
// rows); at 4 + 4 bytes of workspace per point the whole extraction moves a few bytes per grid point (DESIGN 4.7 gives the measured rate).
#include "aon_launch.h"

namespace aon {

constexpr int kMcTile = 1024;
constexpr int kMcThreads = 256;

// Bourke's triangle table: up to 5 triangles per case as edge triples, -1 terminated
__constant__ int8_t kMcTri[256][16] = {
    {-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,8,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,1,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,8,3,9,8,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,8,3,1,2,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {9,2,10,0,2,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {2,8,3,2,10,8,10,9,8,-1,-1,-1,-1,-1,-1,-1},
    {3,11,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,11,2,8,11,0,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,9,0,2,3,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,11,2,1,9,11,9,8,11,-1,-1,-1,-1,-1,-1,-1},
    {3,10,1,11,10,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,10,1,0,8,10,8,11,10,-1,-1,-1,-1,-1,-1,-1}, {3,9,0,3,11,9,11,10,9,-1,-1,-1,-1,-1,-1,-1}, {9,8,10,10,8,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,7,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {4,3,0,7,3,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,1,9,8,4,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {4,1,9,4,7,1,7,3,1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,8,4,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {3,4,7,3,0,4,1,2,10,-1,-1,-1,-1,-1,-1,-1}, {9,2,10,9,0,2,8,4,7,-1,-1,-1,-1,-1,-1,-1}, {2,10,9,2,9,7,2,7,3,7,9,4,-1,-1,-1,-1},
    {8,4,7,3,11,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {11,4,7,11,2,4,2,0,4,-1,-1,-1,-1,-1,-1,-1}, {9,0,1,8,4,7,2,3,11,-1,-1,-1,-1,-1,-1,-1}, {4,7,11,9,4,11,9,11,2,9,2,1,-1,-1,-1,-1},
    {3,10,1,3,11,10,7,8,4,-1,-1,-1,-1,-1,-1,-1}, {1,11,10,1,4,11,1,0,4,7,11,4,-1,-1,-1,-1}, {4,7,8,9,0,11,9,11,10,11,0,3,-1,-1,-1,-1}, {4,7,11,4,11,9,9,11,10,-1,-1,-1,-1,-1,-1,-1},
    {9,5,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {9,5,4,0,8,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,5,4,1,5,0,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {8,5,4,8,3,5,3,1,5,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,9,5,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {3,0,8,1,2,10,4,9,5,-1,-1,-1,-1,-1,-1,-1}, {5,2,10,5,4,2,4,0,2,-1,-1,-1,-1,-1,-1,-1}, {2,10,5,3,2,5,3,5,4,3,4,8,-1,-1,-1,-1},
    {9,5,4,2,3,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,11,2,0,8,11,4,9,5,-1,-1,-1,-1,-1,-1,-1}, {0,5,4,0,1,5,2,3,11,-1,-1,-1,-1,-1,-1,-1}, {2,1,5,2,5,8,2,8,11,4,8,5,-1,-1,-1,-1},
    {10,3,11,10,1,3,9,5,4,-1,-1,-1,-1,-1,-1,-1}, {4,9,5,0,8,1,8,10,1,8,11,10,-1,-1,-1,-1}, {5,4,0,5,0,11,5,11,10,11,0,3,-1,-1,-1,-1}, {5,4,8,5,8,10,10,8,11,-1,-1,-1,-1,-1,-1,-1},
    {9,7,8,5,7,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {9,3,0,9,5,3,5,7,3,-1,-1,-1,-1,-1,-1,-1}, {0,7,8,0,1,7,1,5,7,-1,-1,-1,-1,-1,-1,-1}, {1,5,3,3,5,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,7,8,9,5,7,10,1,2,-1,-1,-1,-1,-1,-1,-1}, {10,1,2,9,5,0,5,3,0,5,7,3,-1,-1,-1,-1}, {8,0,2,8,2,5,8,5,7,10,5,2,-1,-1,-1,-1}, {2,10,5,2,5,3,3,5,7,-1,-1,-1,-1,-1,-1,-1},
    {7,9,5,7,8,9,3,11,2,-1,-1,-1,-1,-1,-1,-1}, {9,5,7,9,7,2,9,2,0,2,7,11,-1,-1,-1,-1}, {2,3,11,0,1,8,1,7,8,1,5,7,-1,-1,-1,-1}, {11,2,1,11,1,7,7,1,5,-1,-1,-1,-1,-1,-1,-1},
    {9,5,8,8,5,7,10,1,3,10,3,11,-1,-1,-1,-1}, {5,7,0,5,0,9,7,11,0,1,0,10,11,10,0,-1}, {11,10,0,11,0,3,10,5,0,8,0,7,5,7,0,-1}, {11,10,5,7,11,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {10,6,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,8,3,5,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {9,0,1,5,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,8,3,1,9,8,5,10,6,-1,-1,-1,-1,-1,-1,-1},
    {1,6,5,2,6,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,6,5,1,2,6,3,0,8,-1,-1,-1,-1,-1,-1,-1}, {9,6,5,9,0,6,0,2,6,-1,-1,-1,-1,-1,-1,-1}, {5,9,8,5,8,2,5,2,6,3,2,8,-1,-1,-1,-1},
    {2,3,11,10,6,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {11,0,8,11,2,0,10,6,5,-1,-1,-1,-1,-1,-1,-1}, {0,1,9,2,3,11,5,10,6,-1,-1,-1,-1,-1,-1,-1}, {5,10,6,1,9,2,9,11,2,9,8,11,-1,-1,-1,-1},
    {6,3,11,6,5,3,5,1,3,-1,-1,-1,-1,-1,-1,-1}, {0,8,11,0,11,5,0,5,1,5,11,6,-1,-1,-1,-1}, {3,11,6,0,3,6,0,6,5,0,5,9,-1,-1,-1,-1}, {6,5,9,6,9,11,11,9,8,-1,-1,-1,-1,-1,-1,-1},
    {5,10,6,4,7,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {4,3,0,4,7,3,6,5,10,-1,-1,-1,-1,-1,-1,-1}, {1,9,0,5,10,6,8,4,7,-1,-1,-1,-1,-1,-1,-1}, {10,6,5,1,9,7,1,7,3,7,9,4,-1,-1,-1,-1},
    {6,1,2,6,5,1,4,7,8,-1,-1,-1,-1,-1,-1,-1}, {1,2,5,5,2,6,3,0,4,3,4,7,-1,-1,-1,-1}, {8,4,7,9,0,5,0,6,5,0,2,6,-1,-1,-1,-1}, {7,3,9,7,9,4,3,2,9,5,9,6,2,6,9,-1},
    {3,11,2,7,8,4,10,6,5,-1,-1,-1,-1,-1,-1,-1}, {5,10,6,4,7,2,4,2,0,2,7,11,-1,-1,-1,-1}, {0,1,9,4,7,8,2,3,11,5,10,6,-1,-1,-1,-1}, {9,2,1,9,11,2,9,4,11,7,11,4,5,10,6,-1},
    {8,4,7,3,11,5,3,5,1,5,11,6,-1,-1,-1,-1}, {5,1,11,5,11,6,1,0,11,7,11,4,0,4,11,-1}, {0,5,9,0,6,5,0,3,6,11,6,3,8,4,7,-1}, {6,5,9,6,9,11,4,7,9,7,11,9,-1,-1,-1,-1},
    {10,4,9,6,4,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {4,10,6,4,9,10,0,8,3,-1,-1,-1,-1,-1,-1,-1}, {10,0,1,10,6,0,6,4,0,-1,-1,-1,-1,-1,-1,-1}, {8,3,1,8,1,6,8,6,4,6,1,10,-1,-1,-1,-1},
    {1,4,9,1,2,4,2,6,4,-1,-1,-1,-1,-1,-1,-1}, {3,0,8,1,2,9,2,4,9,2,6,4,-1,-1,-1,-1}, {0,2,4,4,2,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {8,3,2,8,2,4,4,2,6,-1,-1,-1,-1,-1,-1,-1},
    {10,4,9,10,6,4,11,2,3,-1,-1,-1,-1,-1,-1,-1}, {0,8,2,2,8,11,4,9,10,4,10,6,-1,-1,-1,-1}, {3,11,2,0,1,6,0,6,4,6,1,10,-1,-1,-1,-1}, {6,4,1,6,1,10,4,8,1,2,1,11,8,11,1,-1},
    {9,6,4,9,3,6,9,1,3,11,6,3,-1,-1,-1,-1}, {8,11,1,8,1,0,11,6,1,9,1,4,6,4,1,-1}, {3,11,6,3,6,0,0,6,4,-1,-1,-1,-1,-1,-1,-1}, {6,4,8,11,6,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,10,6,7,8,10,8,9,10,-1,-1,-1,-1,-1,-1,-1}, {0,7,3,0,10,7,0,9,10,6,7,10,-1,-1,-1,-1}, {10,6,7,1,10,7,1,7,8,1,8,0,-1,-1,-1,-1}, {10,6,7,10,7,1,1,7,3,-1,-1,-1,-1,-1,-1,-1},
    {1,2,6,1,6,8,1,8,9,8,6,7,-1,-1,-1,-1}, {2,6,9,2,9,1,6,7,9,0,9,3,7,3,9,-1}, {7,8,0,7,0,6,6,0,2,-1,-1,-1,-1,-1,-1,-1}, {7,3,2,6,7,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,3,11,10,6,8,10,8,9,8,6,7,-1,-1,-1,-1}, {2,0,7,2,7,11,0,9,7,6,7,10,9,10,7,-1}, {1,8,0,1,7,8,1,10,7,6,7,10,2,3,11,-1}, {11,2,1,11,1,7,10,6,1,6,7,1,-1,-1,-1,-1},
    {8,9,6,8,6,7,9,1,6,11,6,3,1,3,6,-1}, {0,9,1,11,6,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {7,8,0,7,0,6,3,11,0,11,6,0,-1,-1,-1,-1}, {7,11,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,6,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {3,0,8,11,7,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,1,9,11,7,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {8,1,9,8,3,1,11,7,6,-1,-1,-1,-1,-1,-1,-1},
    {10,1,2,6,11,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,2,10,3,0,8,6,11,7,-1,-1,-1,-1,-1,-1,-1}, {2,9,0,2,10,9,6,11,7,-1,-1,-1,-1,-1,-1,-1}, {6,11,7,2,10,3,10,8,3,10,9,8,-1,-1,-1,-1},
    {7,2,3,6,2,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {7,0,8,7,6,0,6,2,0,-1,-1,-1,-1,-1,-1,-1}, {2,7,6,2,3,7,0,1,9,-1,-1,-1,-1,-1,-1,-1}, {1,6,2,1,8,6,1,9,8,8,7,6,-1,-1,-1,-1},
    {10,7,6,10,1,7,1,3,7,-1,-1,-1,-1,-1,-1,-1}, {10,7,6,1,7,10,1,8,7,1,0,8,-1,-1,-1,-1}, {0,3,7,0,7,10,0,10,9,6,10,7,-1,-1,-1,-1}, {7,6,10,7,10,8,8,10,9,-1,-1,-1,-1,-1,-1,-1},
    {6,8,4,11,8,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {3,6,11,3,0,6,0,4,6,-1,-1,-1,-1,-1,-1,-1}, {8,6,11,8,4,6,9,0,1,-1,-1,-1,-1,-1,-1,-1}, {9,4,6,9,6,3,9,3,1,11,3,6,-1,-1,-1,-1},
    {6,8,4,6,11,8,2,10,1,-1,-1,-1,-1,-1,-1,-1}, {1,2,10,3,0,11,0,6,11,0,4,6,-1,-1,-1,-1}, {4,11,8,4,6,11,0,2,9,2,10,9,-1,-1,-1,-1}, {10,9,3,10,3,2,9,4,3,11,3,6,4,6,3,-1},
    {8,2,3,8,4,2,4,6,2,-1,-1,-1,-1,-1,-1,-1}, {0,4,2,4,6,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {1,9,0,2,3,4,2,4,6,4,3,8,-1,-1,-1,-1}, {1,9,4,1,4,2,2,4,6,-1,-1,-1,-1,-1,-1,-1},
    {8,1,3,8,6,1,8,4,6,6,10,1,-1,-1,-1,-1}, {10,1,0,10,0,6,6,0,4,-1,-1,-1,-1,-1,-1,-1}, {4,6,3,4,3,8,6,10,3,0,3,9,10,9,3,-1}, {10,9,4,6,10,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,9,5,7,6,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,8,3,4,9,5,11,7,6,-1,-1,-1,-1,-1,-1,-1}, {5,0,1,5,4,0,7,6,11,-1,-1,-1,-1,-1,-1,-1}, {11,7,6,8,3,4,3,5,4,3,1,5,-1,-1,-1,-1},
    {9,5,4,10,1,2,7,6,11,-1,-1,-1,-1,-1,-1,-1}, {6,11,7,1,2,10,0,8,3,4,9,5,-1,-1,-1,-1}, {7,6,11,5,4,10,4,2,10,4,0,2,-1,-1,-1,-1}, {3,4,8,3,5,4,3,2,5,10,5,2,11,7,6,-1},
    {7,2,3,7,6,2,5,4,9,-1,-1,-1,-1,-1,-1,-1}, {9,5,4,0,8,6,0,6,2,6,8,7,-1,-1,-1,-1}, {3,6,2,3,7,6,1,5,0,5,4,0,-1,-1,-1,-1}, {6,2,8,6,8,7,2,1,8,4,8,5,1,5,8,-1},
    {9,5,4,10,1,6,1,7,6,1,3,7,-1,-1,-1,-1}, {1,6,10,1,7,6,1,0,7,8,7,0,9,5,4,-1}, {4,0,10,4,10,5,0,3,10,6,10,7,3,7,10,-1}, {7,6,10,7,10,8,5,4,10,4,8,10,-1,-1,-1,-1},
    {6,9,5,6,11,9,11,8,9,-1,-1,-1,-1,-1,-1,-1}, {3,6,11,0,6,3,0,5,6,0,9,5,-1,-1,-1,-1}, {0,11,8,0,5,11,0,1,5,5,6,11,-1,-1,-1,-1}, {6,11,3,6,3,5,5,3,1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,9,5,11,9,11,8,11,5,6,-1,-1,-1,-1}, {0,11,3,0,6,11,0,9,6,5,6,9,1,2,10,-1}, {11,8,5,11,5,6,8,0,5,10,5,2,0,2,5,-1}, {6,11,3,6,3,5,2,10,3,10,5,3,-1,-1,-1,-1},
    {5,8,9,5,2,8,5,6,2,3,8,2,-1,-1,-1,-1}, {9,5,6,9,6,0,0,6,2,-1,-1,-1,-1,-1,-1,-1}, {1,5,8,1,8,0,5,6,8,3,8,2,6,2,8,-1}, {1,5,6,2,1,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,3,6,1,6,10,3,8,6,5,6,9,8,9,6,-1}, {10,1,0,10,0,6,9,5,0,5,6,0,-1,-1,-1,-1}, {0,3,8,5,6,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {10,5,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,5,10,7,5,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {11,5,10,11,7,5,8,3,0,-1,-1,-1,-1,-1,-1,-1}, {5,11,7,5,10,11,1,9,0,-1,-1,-1,-1,-1,-1,-1}, {10,7,5,10,11,7,9,8,1,8,3,1,-1,-1,-1,-1},
    {11,1,2,11,7,1,7,5,1,-1,-1,-1,-1,-1,-1,-1}, {0,8,3,1,2,7,1,7,5,7,2,11,-1,-1,-1,-1}, {9,7,5,9,2,7,9,0,2,2,11,7,-1,-1,-1,-1}, {7,5,2,7,2,11,5,9,2,3,2,8,9,8,2,-1},
    {2,5,10,2,3,5,3,7,5,-1,-1,-1,-1,-1,-1,-1}, {8,2,0,8,5,2,8,7,5,10,2,5,-1,-1,-1,-1}, {9,0,1,5,10,3,5,3,7,3,10,2,-1,-1,-1,-1}, {9,8,2,9,2,1,8,7,2,10,2,5,7,5,2,-1},
    {1,3,5,3,7,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,8,7,0,7,1,1,7,5,-1,-1,-1,-1,-1,-1,-1}, {9,0,3,9,3,5,5,3,7,-1,-1,-1,-1,-1,-1,-1}, {9,8,7,5,9,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {5,8,4,5,10,8,10,11,8,-1,-1,-1,-1,-1,-1,-1}, {5,0,4,5,11,0,5,10,11,11,3,0,-1,-1,-1,-1}, {0,1,9,8,4,10,8,10,11,10,4,5,-1,-1,-1,-1}, {10,11,4,10,4,5,11,3,4,9,4,1,3,1,4,-1},
    {2,5,1,2,8,5,2,11,8,4,5,8,-1,-1,-1,-1}, {0,4,11,0,11,3,4,5,11,2,11,1,5,1,11,-1}, {0,2,5,0,5,9,2,11,5,4,5,8,11,8,5,-1}, {9,4,5,2,11,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,5,10,3,5,2,3,4,5,3,8,4,-1,-1,-1,-1}, {5,10,2,5,2,4,4,2,0,-1,-1,-1,-1,-1,-1,-1}, {3,10,2,3,5,10,3,8,5,4,5,8,0,1,9,-1}, {5,10,2,5,2,4,1,9,2,9,4,2,-1,-1,-1,-1},
    {8,4,5,8,5,3,3,5,1,-1,-1,-1,-1,-1,-1,-1}, {0,4,5,1,0,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {8,4,5,8,5,3,9,0,5,0,3,5,-1,-1,-1,-1}, {9,4,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,11,7,4,9,11,9,10,11,-1,-1,-1,-1,-1,-1,-1}, {0,8,3,4,9,7,9,11,7,9,10,11,-1,-1,-1,-1}, {1,10,11,1,11,4,1,4,0,7,4,11,-1,-1,-1,-1}, {3,1,4,3,4,8,1,10,4,7,4,11,10,11,4,-1},
    {4,11,7,9,11,4,9,2,11,9,1,2,-1,-1,-1,-1}, {9,7,4,9,11,7,9,1,11,2,11,1,0,8,3,-1}, {11,7,4,11,4,2,2,4,0,-1,-1,-1,-1,-1,-1,-1}, {11,7,4,11,4,2,8,3,4,3,2,4,-1,-1,-1,-1},
    {2,9,10,2,7,9,2,3,7,7,4,9,-1,-1,-1,-1}, {9,10,7,9,7,4,10,2,7,8,7,0,2,0,7,-1}, {3,7,10,3,10,2,7,4,10,1,10,0,4,0,10,-1}, {1,10,2,8,7,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,9,1,4,1,7,7,1,3,-1,-1,-1,-1,-1,-1,-1}, {4,9,1,4,1,7,0,8,1,8,7,1,-1,-1,-1,-1}, {4,0,3,7,4,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {4,8,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,10,8,10,11,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {3,0,9,3,9,11,11,9,10,-1,-1,-1,-1,-1,-1,-1}, {0,1,10,0,10,8,8,10,11,-1,-1,-1,-1,-1,-1,-1}, {3,1,10,11,3,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,11,1,11,9,9,11,8,-1,-1,-1,-1,-1,-1,-1}, {3,0,9,3,9,11,1,2,9,2,11,9,-1,-1,-1,-1}, {0,2,11,8,0,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {3,2,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,3,8,2,8,10,10,8,9,-1,-1,-1,-1,-1,-1,-1}, {9,10,2,0,9,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {2,3,8,2,8,10,0,1,8,1,10,8,-1,-1,-1,-1}, {1,10,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,3,8,9,1,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,9,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {0,3,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1}, {-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
};

// cube corner c at (di, dj, dk): 0 (0,0,0) 1 (1,0,0) 2 (1,1,0) 3 (0,1,0) 4 (0,0,1) 5 (1,0,1) 6 (1,1,1) 7 (0,1,1);
// edge e runs from corner kMcEdgeOwner[e] (as an offset) along axis kMcEdgeAxis[e]
__constant__ int8_t kMcEdgeOff[12][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 0}, {0, 0, 1}, {1, 0, 1},
                                         {0, 1, 1}, {0, 0, 1}, {0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
__constant__ int8_t kMcEdgeAxis[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};

struct McGrid {
  const float* v;
  int64_t nx, ny, nz;
  float level;
};

__device__ __forceinline__ int mc_ntri(int cs) {   // triangles of a case (the table row's length / 3)
  int n = 0;
#pragma unroll
  for (int t = 0; t < 5; ++t) n += kMcTri[cs][3 * t] >= 0 ? 1 : 0;
  return n;
}

// (block_excl_scan: aon_common.h)

// (a) per point: flags = owned-edge bits (x: 1, y: 2, z: 4) | case << 3 (0 when the point names no cell); lvoff = vertex offset in the tile
__global__ __launch_bounds__(kMcThreads) void mc_classify_kernel(McGrid G, uint16_t* __restrict__ flags, uint16_t* __restrict__ lvoff,
                                                                  int64_t* __restrict__ tile_counts) {
  __shared__ int red[kMcThreads / 64];
  const int64_t P = G.nx * G.ny * G.nz, nyz = G.ny * G.nz;
  const int64_t g0 = (int64_t)blockIdx.x * kMcTile + 4 * threadIdx.x;
  int nv[4] = {0, 0, 0, 0}, nt = 0;
  uint16_t fl[4] = {0, 0, 0, 0};
  auto in = [&](int64_t q) { return G.v[q] > G.level ? 1 : 0; };   // NaN: outside
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t g = g0 + r;
    if (g >= P) break;
    const int64_t i = g / nyz, rem = g - i * nyz, j = rem / G.nz, k = rem - j * G.nz;
    const bool hx = i + 1 < G.nx, hy = j + 1 < G.ny, hz = k + 1 < G.nz;
    const int c0 = in(g);
    int eb = 0, cs = 0;
    if (hx && hy && hz) {
      const int c1 = in(g + nyz), c2 = in(g + nyz + G.nz), c3 = in(g + G.nz);
      const int c4 = in(g + 1), c5 = in(g + nyz + 1), c6 = in(g + nyz + G.nz + 1), c7 = in(g + G.nz + 1);
      cs = c0 | c1 << 1 | c2 << 2 | c3 << 3 | c4 << 4 | c5 << 5 | c6 << 6 | c7 << 7;
      eb = (c0 ^ c1) | (c0 ^ c3) << 1 | (c0 ^ c4) << 2;
    } else {
      if (hx) eb |= c0 ^ in(g + nyz);
      if (hy) eb |= (c0 ^ in(g + G.nz)) << 1;
      if (hz) eb |= (c0 ^ in(g + 1)) << 2;
    }
    fl[r] = (uint16_t)(eb | cs << 3);
    nv[r] = __builtin_popcount(eb);
    nt += mc_ntri(cs);
  }
  int vtot, ttot;
  int run = block_excl_scan<int>(nv[0] + nv[1] + nv[2] + nv[3], vtot, red);
  block_excl_scan<int>(nt, ttot, red);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t g = g0 + r;
    if (g >= P) break;
    flags[g] = fl[r];
    lvoff[g] = (uint16_t)run;
    run += nv[r];
  }
  if (threadIdx.x == 0) { tile_counts[2 * blockIdx.x] = vtot; tile_counts[2 * blockIdx.x + 1] = ttot; }
}

// (b) one workgroup: exclusive int64 offsets of the tiles' vertex and triangle counts, in tile order; totals = (V, F)
__global__ __launch_bounds__(kMcThreads) void mc_scan_kernel(const int64_t* __restrict__ tile_counts, int64_t ntiles, int64_t* __restrict__ offs,
                                                             int64_t* __restrict__ totals) {
  __shared__ int64_t red[kMcThreads / 64];
  constexpr int kPer = 8;
  int64_t carry_v = 0, carry_t = 0;
  for (int64_t base = 0; base < ntiles; base += (int64_t)kMcThreads * kPer) {
    const int64_t t0 = base + (int64_t)threadIdx.x * kPer;
    int64_t cv[kPer], ct[kPer], sv = 0, st = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const bool ok = t0 + r < ntiles;
      cv[r] = ok ? tile_counts[2 * (t0 + r)] : 0;
      ct[r] = ok ? tile_counts[2 * (t0 + r) + 1] : 0;
      sv += cv[r]; st += ct[r];
    }
    int64_t tv, tt;
    int64_t rv = carry_v + block_excl_scan<int64_t>(sv, tv, red);
    int64_t rt = carry_t + block_excl_scan<int64_t>(st, tt, red);
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      if (t0 + r < ntiles) { offs[2 * (t0 + r)] = rv; offs[2 * (t0 + r) + 1] = rt; }
      rv += cv[r]; rt += ct[r];
    }
    carry_v += tv; carry_t += tt;
  }
  if (threadIdx.x == 0) { totals[0] = carry_v; totals[1] = carry_t; }
}

struct McOut {
  float lo[3], step[3];
  float* verts; int64_t vcap;   // (vcap, 3)
  int* faces; int64_t fcap;     // (fcap, 3)
};

__device__ __forceinline__ float mc_coord(const McOut& o, int a, int64_t idx) { return __fadd_rn(o.lo[a], __fmul_rn((float)idx, o.step[a])); }

// (c) vertices and faces of a tile at the scanned offsets; writes beyond the caller's capacities are dropped (the host checks V, F first)
__global__ __launch_bounds__(kMcThreads) void mc_emit_kernel(McGrid G, McOut o, const uint16_t* __restrict__ flags, const uint16_t* __restrict__ lvoff,
                                                             const int64_t* __restrict__ offs) {
  __shared__ int red[kMcThreads / 64];
  const int64_t P = G.nx * G.ny * G.nz, nyz = G.ny * G.nz;
  const int64_t g0 = (int64_t)blockIdx.x * kMcTile + 4 * threadIdx.x;
  uint16_t fl[4] = {0, 0, 0, 0};
  int nt[4] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (g0 + r >= P) break;
    fl[r] = flags[g0 + r];
    nt[r] = mc_ntri(fl[r] >> 3);
  }
  int ttot;
  int frun = block_excl_scan<int>(nt[0] + nt[1] + nt[2] + nt[3], ttot, red);
  const int64_t vbase = offs[2 * blockIdx.x], fbase = offs[2 * blockIdx.x + 1];
  const int64_t stride[3] = {nyz, G.nz, 1};
  auto vid_of = [&](int64_t q, int axis) {   // vertex on the +axis edge of point q
    const int f = flags[q];
    return offs[2 * (q / kMcTile)] + lvoff[q] + __builtin_popcount(f & 7 & ((1 << axis) - 1));
  };
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t g = g0 + r;
    if (g >= P) break;
    const int f = fl[r];
    const int64_t idx[3] = {g / nyz, (g / G.nz) % G.ny, g % G.nz};
    // vertices of the owned edges
    if (f & 7) {
      const float v0 = G.v[g];
      int64_t vid = vbase + lvoff[g];
      for (int a = 0; a < 3; ++a) {
        if (!((f >> a) & 1)) continue;
        const float v1 = G.v[g + stride[a]];
        const float x0 = mc_coord(o, a, idx[a]), x1 = mc_coord(o, a, idx[a] + 1);
        float pa;
        if (v1 != v1) pa = x0;          // NaN endpoint: outside, the vertex sits on the inside one
        else if (v0 != v0) pa = x1;
        else {
          const float t = __fdiv_rn(__fsub_rn(G.level, v0), __fsub_rn(v1, v0));
          pa = __fadd_rn(x0, __fmul_rn(t, __fsub_rn(x1, x0)));
        }
        if (vid < o.vcap) {
          float* p = o.verts + 3 * vid;
          p[0] = a == 0 ? pa : mc_coord(o, 0, idx[0]);
          p[1] = a == 1 ? pa : mc_coord(o, 1, idx[1]);
          p[2] = a == 2 ? pa : mc_coord(o, 2, idx[2]);
        }
        ++vid;
      }
    }
    // faces of the cell this point names
    const int cs = f >> 3;
    int64_t fid = fbase + frun;
    for (int t = 0; t < nt[r]; ++t, ++fid) {
      int id[3];
      for (int s = 0; s < 3; ++s) {
        const int e = kMcTri[cs][3 * t + s];
        const int64_t q = g + kMcEdgeOff[e][0] * nyz + kMcEdgeOff[e][1] * G.nz + kMcEdgeOff[e][2];
        id[s] = (int)vid_of(q, kMcEdgeAxis[e]);
      }
      if (fid < o.fcap) {   // table order (a, b, c) -> (a, c, b): normals from high values to low
        int* p = o.faces + 3 * fid;
        p[0] = id[0]; p[1] = id[2]; p[2] = id[1];
      }
    }
    frun += nt[r];
  }
}

// ---- host side ----
// workspace: totals (2 x int64) | tile counts (2 T int64) | tile offsets (2 T int64) | flags (P x u16) | in-tile vertex offsets (P x u16)
static int64_t mc_tiles(const int64_t* d) { return (d[0] * d[1] * d[2] + kMcTile - 1) / kMcTile; }
int64_t mc_workspace_bytes(const int64_t* d) {
  const int64_t P = d[0] * d[1] * d[2], T = mc_tiles(d);
  return 16 + 32 * T + ((4 * P + 15) & ~(int64_t)15);
}

static hipError_t mc_front(const float* grid, const int64_t* d, float level, char* ws, hipStream_t stream, McGrid& G) {
  const int64_t P = d[0] * d[1] * d[2], T = mc_tiles(d);
  int64_t* totals = reinterpret_cast<int64_t*>(ws);
  int64_t* counts = totals + 2;
  int64_t* offs = counts + 2 * T;
  uint16_t* flags = reinterpret_cast<uint16_t*>(offs + 2 * T);
  uint16_t* lvoff = flags + P;
  G = McGrid{grid, d[0], d[1], d[2], level};
  mc_classify_kernel<<<dim3((unsigned)T), dim3(kMcThreads), 0, stream>>>(G, flags, lvoff, counts);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  mc_scan_kernel<<<dim3(1), dim3(kMcThreads), 0, stream>>>(counts, T, offs, totals);
  return hipGetLastError();
}

// (a) + (b), then V and F to the host (synchronises the stream)
hipError_t launch_mc_count(const float* grid, const int64_t* d, float level, void* ws, hipStream_t stream, int64_t* counts2_host) {
  McGrid G;
  if (hipError_t e = mc_front(grid, d, level, static_cast<char*>(ws), stream, G); e != hipSuccess) return e;
  if (hipError_t e = hipMemcpyAsync(counts2_host, ws, 16, hipMemcpyDeviceToHost, stream); e != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

// (a) + (b) + (c): the whole mesh into verts (vcap, 3) / faces (fcap, 3)
hipError_t launch_mc(const float* grid, const int64_t* d, float level, const float* lo, const float* step, void* ws, float* verts, int64_t vcap,
                     int* faces, int64_t fcap, hipStream_t stream) {
  McGrid G;
  char* w = static_cast<char*>(ws);
  if (hipError_t e = mc_front(grid, d, level, w, stream, G); e != hipSuccess) return e;
  const int64_t P = d[0] * d[1] * d[2], T = mc_tiles(d);
  const int64_t* offs = reinterpret_cast<const int64_t*>(w) + 2 + 2 * T;
  const uint16_t* flags = reinterpret_cast<const uint16_t*>(offs + 2 * T);
  McOut o{};
  for (int a = 0; a < 3; ++a) { o.lo[a] = lo[a]; o.step[a] = step[a]; }
  o.verts = verts; o.vcap = vcap; o.faces = faces; o.fcap = fcap;
  mc_emit_kernel<<<dim3((unsigned)T), dim3(kMcThreads), 0, stream>>>(G, o, flags, flags + P, offs);
  return hipGetLastError();
}

}  // namespace aon
