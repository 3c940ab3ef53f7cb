/* Prints aad_launch_policy.h's window_stats_table for the rows on stdin, one line each (tests/test_window_stats_host.py).
 *   T windows out_channels stats_address
 *     -> ok bytes */
#include <cstdio>

#include "aad_launch_policy.h"

int main()
{
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind != 'T') return 1;
    unsigned long long windows, address;
    unsigned channels;
    if (scanf("%llu %u %llu", &windows, &channels, &address) != 3) return 1;
    const aad::WindowStatsTable t = aad::window_stats_table(windows, channels, address);
    printf("%d %llu\n", (int)t.ok, (unsigned long long)t.bytes);
  }
  return 0;
}
