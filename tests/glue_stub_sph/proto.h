/* tests/glue_stub_sph/proto.h -- TEST-ONLY prototypes: those of tests/glue_stub/proto.h and the five of the SPH path (reference
 * proto.h:27,120,138,139,142) */
#ifndef PROTO_H
#define PROTO_H
#include "allvars.h"
void density(void);
void hydro_force(void);
void ngb_treeallocate(int npart);
void ngb_treebuild(void);
void ngb_treefree(void);
void do_box_wrapping(void);
void domain_Decomposition(void);
void force_treeallocate(int maxnodes, int maxpart);
int force_treebuild(int npart);
void force_treefree(void);
void force_treeevaluate_potential(int target, int mode);
void force_treeevaluate_potential_shortrange(int target, int mode);
void force_update_hmax(void);
void force_update_len(void);
void lattice_init(void);
void pmpotential_periodic(void);
void set_softenings(void);
void force_update_pseudoparticles(void);
double get_random_number(int id);
void gravity_forcetest(void);
void gravity_tree(void);
peanokey peano_hilbert_key(int x, int y, int z, int bits);
void peano_hilbert_order(void);
void pm_init_periodic(void);
void pmforce_periodic(void);
double second(void);
double timediff(double t0, double t1);
void endrun(int);
#endif
