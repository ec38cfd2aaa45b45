/* One-task implementations of the third-party calls the reference's SPH path links against (see mpi.h), and loud
 * stops for the symbols that must not be reached.  The project's own text; holds nothing of the reference. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "mpi.h"
#include "gsl/gsl_rng.h"

static void unreachable(const char *name)
{
  fflush(stdout);
  fprintf(stderr, "ref_stubs: %s reached: the one-task harness is wrong\n", name);
  abort();
}

static size_t type_size(MPI_Datatype t)
{
  switch(t)
    {
    case MPI_BYTE: case MPI_CHAR: return 1;
    case MPI_INT: case MPI_UNSIGNED: return sizeof(int);
    case MPI_FLOAT: return sizeof(float);
    case MPI_DOUBLE: return sizeof(double);
    case MPI_LONG: return sizeof(long);
    case MPI_LONG_LONG: return sizeof(long long);
    }
  unreachable("an unknown MPI datatype");
  return 0;
}

static void copy(const void *src, void *dst, size_t bytes)
{
  if(src != MPI_IN_PLACE && src != dst && bytes)
    memmove(dst, src, bytes);
}

int MPI_Allgather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount, MPI_Datatype recvtype, MPI_Comm comm)
{
  (void) recvcount; (void) recvtype; (void) comm;
  copy(sendbuf, recvbuf, (size_t) sendcount * type_size(sendtype));
  return MPI_SUCCESS;
}

int MPI_Allgatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int *recvcounts, const int *displs,
                   MPI_Datatype recvtype, MPI_Comm comm)
{
  (void) recvcounts; (void) comm;
  copy(sendbuf, (char *) recvbuf + (size_t) displs[0] * type_size(recvtype), (size_t) sendcount * type_size(sendtype));
  return MPI_SUCCESS;
}

int MPI_Allreduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype datatype, MPI_Op op, MPI_Comm comm)
{
  (void) op; (void) comm;                     /* sum, minimum, maximum over one task: the task's own value */
  copy(sendbuf, recvbuf, (size_t) count * type_size(datatype));
  return MPI_SUCCESS;
}

int MPI_Reduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype datatype, MPI_Op op, int root, MPI_Comm comm)
{
  (void) op; (void) root; (void) comm;
  copy(sendbuf, recvbuf, (size_t) count * type_size(datatype));
  return MPI_SUCCESS;
}

int MPI_Bcast(void *buffer, int count, MPI_Datatype datatype, int root, MPI_Comm comm)
{
  (void) buffer; (void) count; (void) datatype; (void) root; (void) comm;
  return MPI_SUCCESS;
}

int MPI_Barrier(MPI_Comm comm)
{
  (void) comm;
  return MPI_SUCCESS;
}

double MPI_Wtime(void)
{
  return (double) clock() / CLOCKS_PER_SEC;
}

int MPI_Sendrecv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, int dest, int sendtag, void *recvbuf, int recvcount,
                 MPI_Datatype recvtype, int source, int recvtag, MPI_Comm comm, MPI_Status *status)
{
  (void) sendbuf; (void) sendcount; (void) sendtype; (void) dest; (void) sendtag; (void) recvbuf; (void) recvcount;
  (void) recvtype; (void) source; (void) recvtag; (void) comm; (void) status;
  unreachable("MPI_Sendrecv");
  return 1;
}

int MPI_Ssend(const void *buf, int count, MPI_Datatype datatype, int dest, int tag, MPI_Comm comm)
{
  (void) buf; (void) count; (void) datatype; (void) dest; (void) tag; (void) comm;
  unreachable("MPI_Ssend");
  return 1;
}

int MPI_Recv(void *buf, int count, MPI_Datatype datatype, int source, int tag, MPI_Comm comm, MPI_Status *status)
{
  (void) buf; (void) count; (void) datatype; (void) source; (void) tag; (void) comm; (void) status;
  unreachable("MPI_Recv");
  return 1;
}

int MPI_Abort(MPI_Comm comm, int errorcode)
{
  (void) comm;
  fflush(stdout);
  fprintf(stderr, "ref_stubs: MPI_Abort(%d): the reference stopped itself\n", errorcode);
  abort();
}

int MPI_Finalize(void)
{
  unreachable("MPI_Finalize");                /* the driver ends by returning from main(), never through the reference */
  return 1;
}

/* the reference's own file and parameter I/O helpers and its random number source: not on the SPH path */
size_t my_fwrite(void *ptr, size_t size, size_t nmemb, FILE *stream)
{
  (void) ptr; (void) size; (void) nmemb; (void) stream;
  unreachable("my_fwrite");
  return 0;
}

size_t my_fread(void *ptr, size_t size, size_t nmemb, FILE *stream)
{
  (void) ptr; (void) size; (void) nmemb; (void) stream;
  unreachable("my_fread");
  return 0;
}

double gsl_rng_uniform(const gsl_rng *r)
{
  (void) r;
  unreachable("gsl_rng_uniform");
  return 0;
}
