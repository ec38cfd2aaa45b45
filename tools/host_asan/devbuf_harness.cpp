// The owners of device resources (csrc/devbuf.hpp: DevBuf, DevEvent, DevStream) under AddressSanitizer + UndefinedBehaviorSanitizer
// and the leak check, with no HIP runtime: the five runtime calls the header makes are defined here over malloc / free.  They count
// the live objects of every kind and can be told to fail their k-th call.  After every case nothing is alive.
// tests/test_devbuf_asan.py builds and runs this file; it includes nothing of the GPU.
#include "devbuf.hpp"
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

static long live_bufs = 0, live_events = 0, live_streams = 0;
static long mallocs = 0, fail_malloc = 0;   // calls so far; the call with this number fails (0: none)
static long events = 0, fail_event = 0;

extern "C" hipError_t hipMalloc(void **p, size_t bytes)
{
  if(++mallocs == fail_malloc)
    return hipErrorOutOfMemory;
  *p = malloc(bytes ? bytes : 1);
  if(!*p)
    abort();
  live_bufs++;
  return hipSuccess;
}
extern "C" hipError_t hipFree(void *p)
{
  if(p)
    live_bufs--;
  free(p);
  return hipSuccess;
}
extern "C" hipError_t hipEventCreate(hipEvent_t *e)
{
  if(++events == fail_event)
    return hipErrorOutOfMemory;
  *e = static_cast<hipEvent_t>(malloc(1));
  live_events++;
  return hipSuccess;
}
extern "C" hipError_t hipEventDestroy(hipEvent_t e)
{
  live_events--;
  free(e);
  return hipSuccess;
}
extern "C" hipError_t hipStreamDestroy(hipStream_t s)
{
  live_streams--;
  free(s);
  return hipSuccess;
}
// a stream as hipExtStreamCreateWithCUMask hands it out: a bare handle that somebody has to adopt
static hipStream_t bare_stream()
{
  live_streams++;
  return static_cast<hipStream_t>(malloc(1));
}

static_assert(!std::is_copy_constructible<DevBuf<double>>::value && !std::is_copy_assignable<DevBuf<double>>::value, "DevBuf copies");
static_assert(!std::is_copy_constructible<DevEvent>::value && !std::is_copy_assignable<DevEvent>::value, "DevEvent copies");
static_assert(!std::is_copy_constructible<DevStream>::value && !std::is_copy_assignable<DevStream>::value, "DevStream copies");
static_assert(std::is_nothrow_move_constructible<DevBuf<double>>::value && std::is_nothrow_move_constructible<DevEvent>::value, "moves");
static_assert(sizeof(DevBuf<double>) == sizeof(double *) + sizeof(size_t), "DevBuf is a pointer and a capacity");
static_assert(sizeof(DevEvent) == sizeof(hipEvent_t) && sizeof(DevStream) == sizeof(hipStream_t), "a handle and nothing else");

static int cases = 0;
#define CHECK(x)                                                         \
  do                                                                     \
    if(!(x))                                                             \
      {                                                                  \
        printf("FAILED: case %d, line %d: %s\n", cases, __LINE__, #x);   \
        exit(1);                                                         \
      }                                                                  \
  while(0)
// the end of a case: nothing is alive, no failure is armed
static void done()
{
  CHECK(live_bufs == 0 && live_events == 0 && live_streams == 0);
  fail_malloc = fail_event = 0;
  cases++;
}
static size_t grown(size_t n) { return n + n / 16 + 64; }
// every element can be written (the sanitizer sees a write past what hipMalloc was asked for)
template <typename T> static void fill(DevBuf<T> &b)
{
  for(size_t i = 0; i < b.cap; i++)
    b.p[i] = T(i);
}

static void ensure_grows_and_stays()
{
  DevBuf<double> b;
  CHECK(!b.p && b.cap == 0 && b.ensure(0) == 0 && !b.p);
  CHECK(b.ensure(1000) == 0 && b.p && b.cap == grown(1000));
  fill(b);
  double *p = b.p;
  CHECK(b.ensure(1) == 0 && b.ensure(grown(1000)) == 0 && b.p == p && b.cap == grown(1000));   // no grow: the same memory
  CHECK(b.ensure(grown(1000) + 1) == 0 && b.cap == grown(grown(1000) + 1) && live_bufs == 1);  // a grow frees the old block
  fill(b);
}
static void ensure_fails()
{
  DevBuf<int> b;
  CHECK(b.ensure(10) == 0);
  fail_malloc = mallocs + 1;
  CHECK(b.ensure(1000) == -1 && !b.p && b.cap == 0 && live_bufs == 0);   // empty ...
  CHECK(b.ensure(5) == 0 && b.cap == grown(5));                          // ... and usable
  fill(b);
}
static void release_twice()
{
  DevBuf<char> b;
  CHECK(b.ensure(3) == 0);
  b.release();
  CHECK(!b.p && b.cap == 0 && live_bufs == 0);
  b.release();
  b.release();
}
static void move_construction()
{
  DevBuf<double> a;
  CHECK(a.ensure(7) == 0);
  double *p = a.p;
  DevBuf<double> b(std::move(a));
  CHECK(!a.p && a.cap == 0 && b.p == p && b.cap == grown(7) && live_bufs == 1);
  DevBuf<double> e(std::move(a));   // of an empty one
  CHECK(!e.p && e.cap == 0);
}
static void move_assignment(bool target_full)
{
  DevBuf<double> a, b;
  CHECK(a.ensure(7) == 0 && (!target_full || b.ensure(9) == 0));
  double *p = a.p;
  b = std::move(a);
  CHECK(!a.p && a.cap == 0 && b.p == p && b.cap == grown(7) && live_bufs == 1);   // what b held is freed
  b = std::move(a);   // an empty source empties the target
  CHECK(!b.p && b.cap == 0 && live_bufs == 0);
}
static void self_move_assignment()
{
  DevBuf<double> a;
  CHECK(a.ensure(7) == 0);
  double *p = a.p;
  DevBuf<double> &r = a;
  a = std::move(r);
  CHECK(a.p == p && a.cap == grown(7) && live_bufs == 1);
  fill(a);
  DevEvent e;
  CHECK(e.create() == hipSuccess);
  DevEvent &re = e;
  e = std::move(re);
  CHECK(e && live_events == 1);
}
static void swap()
{
  DevBuf<double> a, b;
  CHECK(a.ensure(7) == 0 && b.ensure(900) == 0);
  double *pa = a.p, *pb = b.p;
  std::swap(a, b);
  CHECK(a.p == pb && a.cap == grown(900) && b.p == pa && b.cap == grown(7) && live_bufs == 2);
  DevBuf<double> e;
  std::swap(a, e);
  CHECK(!a.p && a.cap == 0 && e.p == pb && live_bufs == 2);
}
static void event_vector_grows()
{
  std::vector<DevEvent> v;
  std::vector<hipEvent_t> h;
  for(int i = 0; i < 100; i++)   // through several reallocations
    {
      DevEvent e;
      CHECK(e.create() == hipSuccess);
      h.push_back(e);
      v.push_back(std::move(e));
      CHECK(!e && live_events == i + 1);
    }
  for(int i = 0; i < 100; i++)
    CHECK(v[i] == h[i]);
  fail_event = events + 1;
  DevEvent e;
  CHECK(e.create() != hipSuccess && !e && live_events == 100);
  CHECK(e.create() == hipSuccess && e.create() == hipSuccess && live_events == 101);   // a second create destroys the first event
}
// `if(a.ensure() || b.ensure() || ...) return NOMEM;` with K buffers, the k-th allocation failing
static int early_return(int k)
{
  const int K = 4;
  DevBuf<double> a, b;
  DevBuf<int> c;
  DevBuf<char> d;
  fail_malloc = mallocs + 1 + k;
  if(a.ensure(10) || b.ensure(20) || c.ensure(30) || d.ensure(40))
    {
      CHECK(k < K && live_bufs == k);
      return -1;
    }
  CHECK(k >= K && live_bufs == K);
  return 0;
}
// dd_apply_migration: eight temporaries, one of them optional, take the place of eight members; the f-th allocation fails
struct Columns
{
  DevBuf<double> pos, mass, old, cost, pm;
  DevBuf<int> type;
  DevBuf<unsigned char> act;
  DevBuf<long long> id;
};
static int replace_columns(Columns &m, size_t cap, bool with_pm, long f)
{
  DevBuf<double> pos2, mass2, old2, cost2, pm2;
  DevBuf<int> type2;
  DevBuf<unsigned char> act2;
  DevBuf<long long> id2;
  fail_malloc = mallocs + 1 + f;
  if(pos2.ensure(3 * cap) || mass2.ensure(cap) || old2.ensure(cap) || type2.ensure(cap) || act2.ensure(cap) || id2.ensure(cap) ||
     cost2.ensure(cap) || (with_pm && pm2.ensure(3 * cap)))
    return -1;
  fill(pos2);
  m.cost = std::move(cost2);
  if(with_pm)
    m.pm = std::move(pm2);
  m.pos = std::move(pos2);
  m.mass = std::move(mass2);
  m.old = std::move(old2);
  m.type = std::move(type2);
  m.act = std::move(act2);
  m.id = std::move(id2);
  return 0;
}
static void replace_columns_all_failures(bool with_pm)
{
  const long n = with_pm ? 8 : 7;
  for(long f = 0; f <= n; f++)
    {
      Columns m;
      CHECK(replace_columns(m, 100, with_pm, n) == 0 && live_bufs == n);   // the members hold columns already
      double *before = m.pos.p;
      const int rc = replace_columns(m, 200, with_pm, f);
      CHECK(rc == (f < n ? -1 : 0) && live_bufs == n);   // the temporaries are gone either way
      CHECK(f < n ? (m.pos.p == before && m.pos.cap == grown(300)) : m.pos.cap == grown(600));   // a failed call changes nothing
      fill(m.pos);
    }
}
struct Streams
{
  DevStream pm, walk;
};
static void adopt_then_move()
{
  Streams m;
  for(int round = 0; round < 2; round++)   // the second round replaces streams the members hold
    {
      DevStream sp, sw;
      sp.adopt(bare_stream());
      CHECK(sp && !sw && live_streams == 1 + 2 * round);
      {
        DevStream lost;   // the pair is not complete: the caller returns, what it made goes with it
        lost.adopt(bare_stream());
      }
      CHECK(live_streams == 1 + 2 * round);
      sw.adopt(bare_stream());
      hipStream_t hp = sp, hw = sw;
      m.pm = std::move(sp);
      m.walk = std::move(sw);
      CHECK(!sp && !sw && m.pm == hp && m.walk == hw && live_streams == 2);
    }
  m.pm.adopt(nullptr);
  CHECK(!m.pm && live_streams == 1);
}

int main()
{
  ensure_grows_and_stays(), done();
  ensure_fails(), done();
  release_twice(), done();
  move_construction(), done();
  move_assignment(false), done();
  move_assignment(true), done();
  self_move_assignment(), done();
  swap(), done();
  event_vector_grows(), done();
  for(int k = 0; k <= 4; k++)
    {
      CHECK(early_return(k) == (k < 4 ? -1 : 0));
      done();
    }
  replace_columns_all_failures(false), done();
  replace_columns_all_failures(true), done();
  adopt_then_move(), done();
  printf("%d cases OK\n", cases);
  return 0;
}
