/* ref_cli.cpp -- command-line front end of the reference solver compiled where it lies (test
 * infrastructure only).  usage: ref_cli <bedGraph> <penalty> <db>   (exit status = status code) */
#include <stdio.h>
int PeakSegFPOP_disk(char *, char *, char *);
int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s bedGraph penalty db\n", argv[0]); return 64; }
  return PeakSegFPOP_disk(argv[1], argv[2], argv[3]);
}
