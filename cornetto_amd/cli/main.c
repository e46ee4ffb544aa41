/* main.c — `cornetto <command>` dispatcher; mirrors src/main.c:95-152 of the reference for the
 * panel-creation sub-commands (same names, same exit codes, same 3-line stderr footer), for fixasm
 * (fixasm_main.c), for the evaluation sub-commands asmstats, nx, report and telocontigs (eval_main.c) and for telostats, the reference's
 * scripts/telostats.sh as one sub-command (telostats_main.c), and for qv and trioeval, the k-mer QV and the switch / Hamming error steps of
 * the protocol (qv_main.c, trioeval_main.c).
 * minidot, the one sub-command of the reference outside this build, is not in the usage text and exits
 * with status 1 as unrecognised; telobreaks is built and dispatched below. */
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "cli.h"

static int print_usage(FILE *fp)
{
    fprintf(fp, "Usage: cornetto <command> [options]\n\n");
    fprintf(fp, "commands (MI355X build; minidot is not built):\n");
    fprintf(fp, "   create panel:\n");
    fprintf(fp, "       noboringbits    print no boring bits in an assembly\n");
    fprintf(fp, "       boringbits      print boring bits in an assembly (deprecated)\n");
    fprintf(fp, "       bigenough       find contigs that have sufficient boring bits\n");
    fprintf(fp, "       depth           (stub, as in the reference)\n");
    fprintf(fp, "   telo:\n");
    fprintf(fp, "       telowin         analyse telomere windows in a fasta file\n");
    fprintf(fp, "       telofind        find telomere sequences in a fasta file\n");
    fprintf(fp, "       telobreaks      find telomere sequences inside low-complexity runs\n");
    fprintf(fp, "       telostats       telomere regions at the contig ends (telomere.bed for telocontigs and asmstats)\n");
    fprintf(fp, "       sdust           symmetric DUST (https://github.com/lh3/sdust)\n");
    fprintf(fp, "   assembly toolkit:\n");
    fprintf(fp, "       fixasm          rename and reorient assembly contigs after their alignments to a reference\n");
    fprintf(fp, "   eval:\n");
    fprintf(fp, "       asmstats        calculate assembly statistics\n");
    fprintf(fp, "       nx              nx or ngx plot tables\n");
    fprintf(fp, "       qv              k-mer consensus quality of assemblies against a truth assembly\n");
    fprintf(fp, "       report          generate a report table for one or more assemblies\n");
    fprintf(fp, "       telocontigs     prints contigs from largest to smallest with number of telomeres\n");
    fprintf(fp, "       trioeval        switch and Hamming error of phased assemblies against parental k-mers\n");
    fprintf(fp, "   misc:\n");
    fprintf(fp, "       fa2bed          create a bed file with assembly contig lengths\n");
    fprintf(fp, "       seq             extract reads equal or longer than a threshold from a fastq\n");
    fprintf(fp, "\n");
    fprintf(fp, "       --help, -h      print this help message\n");
    fprintf(fp, "       --version, -V   print version information\n");
    return fp == stdout ? EXIT_SUCCESS : EXIT_FAILURE;
}

int main(int argc, char *argv[])
{
    double realtime0 = cli_realtime();
    int ret = 1;
    if (argc < 2) {
        return print_usage(stderr);
    } else if (strcmp(argv[1], "depth") == 0) {
        ret = depth_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "boringbits") == 0) {
        ret = boringbits_main(argc - 1, argv + 1, 1);
    } else if (strcmp(argv[1], "noboringbits") == 0) {
        ret = boringbits_main(argc - 1, argv + 1, 0);
    } else if (strcmp(argv[1], "telowin") == 0) {
        ret = telomere_windows_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "telobreaks") == 0) {
        ret = telomere_breaks_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "telostats") == 0) {
        ret = telostats_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "telofind") == 0) {
        ret = find_telomere_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "bigenough") == 0) {
        ret = bigenough_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "sdust") == 0) {
        ret = sdust_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "fa2bed") == 0) {
        ret = assbed_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "fixasm") == 0) {
        ret = fixasm_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "nx") == 0) {
        ret = nx_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "report") == 0) {
        ret = report_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "telocontigs") == 0) {
        ret = telocontigs_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "asmstats") == 0) {
        ret = asmstats_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "qv") == 0) {
        ret = qv_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "trioeval") == 0) {
        ret = trioeval_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "seq") == 0) {
        ret = seq_main(argc - 1, argv + 1);
    } else if (strcmp(argv[1], "--version") == 0 || strcmp(argv[1], "-V") == 0) {
        fprintf(stdout, "cornetto %s\n", CORNETTO_VERSION);
        exit(EXIT_SUCCESS);
    } else if (strcmp(argv[1], "--help") == 0 || strcmp(argv[1], "-h") == 0) {
        return print_usage(stdout);
    } else {
        fprintf(stderr, "[cornetto] Unrecognised command %s\n", argv[1]);
        return print_usage(stderr);
    }
    fprintf(stderr, "[%s] Version: %s (MI355X/HIP backend)\n", __func__, CORNETTO_VERSION);
    fprintf(stderr, "[%s] CMD:", __func__);
    for (int i = 0; i < argc; ++i) fprintf(stderr, " %s", argv[i]);
    fprintf(stderr, "\n[%s] Real time: %.3f sec; CPU time: %.3f sec; Peak RAM: %.3f GB\n\n", __func__,
            cli_realtime() - realtime0, cli_cputime(), cli_peakrss() / 1024.0 / 1024.0 / 1024.0);
    /* everything is printed: leave without the orderly teardown of the HIP runtime and of gigabytes of pinned memory
     * (0.1-0.2 s that the kernel does faster) */
    fflush(NULL);
    _exit(ret);
}
