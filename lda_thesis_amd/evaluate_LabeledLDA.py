"""Command-line harness with the flags and the report of /root/reference/evaluate_LabeledLDA.py:110-180
(train Labeled LDA on the GPU, fold the held-out 10 % in, print AUC / one-error / two-error / F1).

    python -m lda_thesis_amd.evaluate_LabeledLDA -f abstracts_data.csv -d 3 -i 4 -s 4 -l 0 -u 1 -a 0.1 -b 0.01
"""
import pickle
from optparse import OptionParser

import numpy as np

from .evaluate import binary_yreal, get_f1, macro_auc_roc, n_error, rates
from .LabeledLDA import split_data, test_it, train_it


def build_parser():
    p = OptionParser()
    p.add_option("-f", dest="file", help="dataset location")
    p.add_option("-d", dest="lvl", type="int", default=3, help="depth of lab level")
    p.add_option("-i", dest="it", type="int", help="# of iterations")
    p.add_option("-s", dest="thinning", type="int", default=0, help="save frequency")
    p.add_option("-l", dest="lower", type="float", default=0, help="lower threshold for dictionary pruning")
    p.add_option("-u", dest="upper", type="float", default=1, help="upper threshold for dictionary pruning")
    p.add_option("-a", dest="alpha", type="float", default=0.1, help="alpha prior")
    p.add_option("-b", dest="beta", type="float", default=0.01, help="beta prior")
    p.add_option("-p", action="store_true", dest="pickle", default=False, help="Save the model as pickle?")
    p.add_option("--device-metrics", action="store_true", dest="device_metrics", default=False,
                 help="rank the labels and compute the four metrics on the GPU (llda_rank_labels)")
    p.add_option("--coherence", dest="coherence", type="int", default=0, metavar="N",
                 help="after the report: UMass coherence of every label's N best words over the training corpus (llda_top_words, "
                      "llda_word_cooc), its mean and the five worst labels")
    p.add_option("--window-coherence", dest="window_coherence", type="int", default=0, metavar="N",
                 help="after the report: C_V coherence (sliding windows of 110 tokens) of every label's N best words over the training "
                      "token lists (llda_top_words, llda_window_cooc), its mean and the five worst labels")
    p.add_option("--label-words", dest="label_words", type="int", default=0, metavar="N",
                 help="after the report: every label's N most distinctive words (relevance --relevance; llda_scored_words) next to its "
                      "N most frequent ones; with --coherence / --window-coherence also the mean coherence of both lists")
    p.add_option("--relevance", dest="relevance", type="float", default=0.6, metavar="L",
                 help="the weight of --label-words between a word's probability under the label (1) and its lift over the corpus (0), "
                      "as in LDAvis; rounded to a fraction with a denominator of at most 8")
    p.add_option("--frex-words", dest="frex_words", type="int", default=0, metavar="N",
                 help="after the report: every label's N FREX words (Bischof and Airoldi 2012; llda_ecdf_ranks, llda_frex_select) next "
                      "to its N most frequent ones")
    p.add_option("--frex-weight", dest="frex_weight", type="float", default=None, metavar="W",
                 help="the weight of --frex-words (default 0.5) and --exclusivity (default 0.7) on a word's exclusivity (1) against its "
                      "probability under the label (0); rounded to a fraction with a denominator of at most 64")
    p.add_option("--exclusivity", dest="exclusivity", type="int", default=0, metavar="N",
                 help="after the report: topic exclusivity, the sum of FREX over every label's N most probable words, its mean and the "
                      "five least exclusive labels")
    p.add_option("--heldout-perplexity", action="store_true", dest="heldout_perplexity", default=False,
                 help="after the report: perplexity of the held-out documents by document completion (every second word of a "
                      "document folded in, the others scored on the GPU: llda_heldout_loglik)")
    p.add_option("--left-to-right", dest="left_to_right", type="int", default=0, metavar="R",
                 help="after the report: perplexity of the held-out documents from the left-to-right estimate of their likelihood "
                      "with R particles (Wallach et al. 2009; llda_left_to_right)")
    p.add_option("--lr-sparse", action="store_true", dest="lr_sparse", default=False,
                 help="with --left-to-right: score every test document against its own labels (the ones the model knows, and "
                      "'root') through the sparse-label kernel (llda_left_to_right_sparse): p(w_d | labels_d), for every K")
    p.add_option("--shortlist", dest="shortlist", type="int", default=0, metavar="M",
                 help="after the report: the same four metrics with the fold-in sampler run on a shortlist of every test document: "
                      "'root' plus the M <= 16 labels with the most credit after one attribution pass (llda_attribute, "
                      "llda_rank_labels, llda_foldin_sparse); a site then costs M + 1 loadings per sweep, not K")
    p.add_option("--heldout-em", dest="heldout_em", type="int", default=0, metavar="ITERS",
                 help="after the report: perplexity of the held-out documents by document completion without random numbers: the "
                      "observed half folded in by ITERS EM steps (llda_attribute, llda_heldout_loglik); with --em-sparse against "
                      "the documents' own labels through the sparse-label kernels (llda_attribute_sparse, llda_heldout_loglik_sparse)")
    p.add_option("--em-foldin", dest="em_foldin", type="int", default=0, metavar="ITERS",
                 help="after the report: the same four metrics for the loads of the deterministic EM fold-in with ITERS steps "
                      "(llda_attribute), ranked and scored on the GPU")
    p.add_option("--em-train", dest="em_train", type="int", default=0, metavar="ITERS",
                 help="fit the model by ITERS passes of deterministic EM (llda_attribute, llda_credit_words, llda_phi_step) in place "
                      "of the Gibbs sweeps of -i / -s, which then only set the fold-in of the test documents")
    p.add_option("--em-sparse", dest="em_sparse", action="store_true", default=False,
                 help="with --em-train: the sparse-label form of the EM fit (llda_attribute_sparse, llda_credit_words_sparse): a site "
                      "reads its document's own labels of phi, not all K; at most 32 labels per document")
    p.add_option("--explain", dest="explain", type="int", default=0, metavar="N",
                 help="after the report: for the first N test documents the suggested labels with the five most-credited words "
                      "of each (llda_attribute)")
    p.add_option("--knn", dest="knn", type="int", default=0, metavar="K",
                 help="after the report: the same four metrics for the votes of the K nearest training documents of every test "
                      "document (Hellinger affinity of the loads; llda_nearest_rows)")
    p.add_option("--similar-labels", dest="similar_labels", type="int", default=0, metavar="N",
                 help="after the report: every label with its N nearest labels by word distribution (llda_nearest_rows)")
    p.add_option("--label-report", action="store_true", dest="label_report", default=False,
                 help="after the report: label-wise evaluation of the test documents (llda_label_metrics): macro-averaged AUC and "
                      "best F1 over the labels, and the ten best and ten worst labels by AUC")
    p.add_option("--label-sets", action="store_true", dest="label_sets", default=False,
                 help="after the report: per-label thresholds tuned for F1 on the even-indexed documents of the test split, then "
                      "micro / macro / example-based F1 of the predicted label sets on its odd-indexed documents (llda_label_sets)")
    return p


def report_labels(model, test, it, thinning):
    """macro figures over the labels and the ten best / ten worst labels by AUC (LabeledLDA.label_report)"""
    known = set(model.vocab)
    r = model.label_report([[x for x in doc if x in known] for doc in test[0]], test[1], it, thinning)
    print("-----------------------------------")
    print("Label-wise evaluation over %d labels (%d without a positive or a negative test document):" % (r["n_labels"], r["skipped"]))
    print("AUC ROC (macro over labels):  ", r["macro_auc"])
    print("best F1 (macro over labels):  ", r["macro_f1"])
    rows = sorted((x for x in r["table"] if x[2] == x[2]), key=lambda x: (-x[2], x[0]))
    for title, part in (("best", rows[:10]), ("worst", rows[::-1][:10])):
        print("ten %s labels by AUC (label, support, AUC, best F1, threshold):" % title)
        for name, support, auc, f1, thr in part:
            print("  %-24s %6d  %.4f  %.4f  %.6g" % (name, support, auc, f1, thr))
    return r


def report_label_sets(model, test, it, thinning):
    """thresholds tuned on the even-indexed test documents, label sets scored on the odd-indexed ones"""
    known = set(model.vocab)
    docs = [[x for x in doc if x in known] for doc in test[0]]
    labels = list(test[1])
    thr = model.tune_thresholds(docs[0::2], labels[0::2], it, thinning)
    print("-----------------------------------")
    print("Label sets: %d thresholds tuned on %d documents, scored on %d:" % (int((~np.isnan(thr)).sum()), len(docs[0::2]), len(docs[1::2])))
    if not docs[1::2]:
        print("  no document to score")
        return None
    r = model.score_test_sets(docs[1::2], labels[1::2], it, thinning)
    print("F1 (micro):              ", r["micro_f1"])
    print("F1 (macro over labels):  ", r["macro_f1"])
    print("F1 (example-based):      ", r["example_f1"])
    return r


def report_knn(model, test, it, thinning, k):
    """the four metrics of the report for the votes of the k nearest training documents (LabeledLDA.score_test_knn)"""
    known = set(model.vocab)
    m = model.score_test_knn([[x for x in doc if x in known] for doc in test[0]], test[1], it, thinning, k=k)
    print("-----------------------------------")
    print("k nearest training documents (k = %d, Hellinger affinity):" % k)
    print("AUC ROC:                 ", m["auc"])
    print("one error:               ", m["one_error"])
    print("two error:               ", m["two_error"])
    print("F1 score (macro average) ", m["f1"])
    return m


def report_similar_labels(model, n):
    """every label with its n nearest labels by word distribution (LabeledLDA.similar_labels)"""
    print("-----------------------------------")
    print("Nearest labels by word distribution (Hellinger affinity, top %d):" % n)
    for name, near in model.similar_labels(n):
        print("  %-24s %s" % (name, "  ".join("%s %.4f" % (other, aff) for other, aff in near)))


def report_em_foldin(model, test, iters):
    """the four metrics of the report for the EM loads of the test documents (LabeledLDA.fold_in_em), through ranking.metrics"""
    from . import ranking
    known = set(model.vocab)
    th = model.fold_in_em([[x for x in doc if x in known] for doc in test[0]], iters=iters)
    m = ranking.metrics(ranking.rank_labels(th, binary_yreal(test[1], model.labelmap), first=1, top_n=0))
    print("-----------------------------------")
    print("EM fold-in, %d steps (no random numbers):" % iters)
    print("AUC ROC:                 ", m["auc"])
    print("one error:               ", m["one_error"])
    print("two error:               ", m["two_error"])
    print("F1 score (macro average) ", m["f1"])
    return m


def report_shortlist(model, test, it, thinning, m):
    """the four metrics of the report for the sampler on root plus the m best-credited labels (LabeledLDA.score_test(shortlist=m))"""
    known = set(model.vocab)
    r = model.score_test([[x for x in doc if x in known] for doc in test[0]], test[1], it, thinning, shortlist=m)
    print("-----------------------------------")
    print("Fold-in on a shortlist of %d labels per document:" % m)
    print("AUC ROC:                 ", r["auc"])
    print("one error:               ", r["one_error"])
    print("two error:               ", r["two_error"])
    print("F1 score (macro average) ", r["f1"])
    return r


def report_explain(model, test, n_docs, iters):
    """for the first n_docs test documents: the suggested labels (LabeledLDA.explain) with the five most-credited words of each"""
    known = set(model.vocab)
    docs = [[x for x in doc if x in known] for doc in test[0][:n_docs]]
    print("-----------------------------------")
    print("Credit attribution of the first %d test documents:" % len(docs))
    for d, (words, credit) in enumerate(model.explain(docs, iters=iters)):
        print("document %d: %d tokens" % (d, sum(f for _, f, _ in words)))
        for label in sorted(credit, key=lambda x: (-credit[x], x)):
            got = {}
            for token, f, shares in words:
                for lab, share in shares:
                    if lab == label:
                        got[token] = got.get(token, 0.0) + f * share
            best = sorted(got, key=lambda t: (-got[t], t))[:5]
            print("  %-24s %8.2f  %s" % (label, credit[label], " ".join(best)))


def known_labels(model, test):
    """the labels of every test document that the model has a topic for"""
    return [[x for x in labs if x in model.labelmap] for labs in test[1]]


def report_left_to_right(model, test, particles, sparse=False):
    """held-out perplexity of the test documents from the left-to-right estimate of p(w_d | phi, alpha); sparse: of p(w_d | labels_d),
    every document against its own labels"""
    r = model.left_to_right(test[0], particles=particles, labels=known_labels(model, test), sparse=True) if sparse else \
        model.left_to_right(test[0], particles=particles)
    print("-----------------------------------")
    print("Held-out perplexity (left-to-right%s, %d particles): " % (", own labels" if sparse else "", particles), r["perplexity"])
    print("  scored tokens %d in %d documents (%d skipped, %d bad tokens), log-likelihood %s"
          % (r["tokens"], r["documents"], r["skipped"], r["bad"], r["loglik"]))
    return r


def report_heldout(model, test, it, thinning):
    """held-out perplexity of the test documents (the words the model knows, as test_it folds them in) by document completion"""
    known = set(model.vocab)
    r = model.heldout_perplexity([[x for x in doc if x in known] for doc in test[0]], it, thinning)
    print("-----------------------------------")
    print("Held-out perplexity (document completion): ", r["perplexity"])
    print("  scored tokens %d in %d documents (%d skipped), log-likelihood %s" % (r["tokens"], r["documents"], r["skipped"], r["loglik"]))
    return r


def report_heldout_em(model, test, iters, sparse=False):
    """held-out perplexity by document completion with the EM fold-in (LabeledLDA.heldout_perplexity_em); sparse: against the
    documents' own labels, through the sparse-label kernels"""
    known = set(model.vocab)
    docs = [[x for x in doc if x in known] for doc in test[0]]
    r = model.heldout_perplexity_em(docs, iters=iters, labels=known_labels(model, test), sparse=True) if sparse else \
        model.heldout_perplexity_em(docs, iters=iters)
    print("-----------------------------------")
    print("Held-out perplexity (document completion, EM fold-in of %d steps%s): " % (iters, ", own labels" if sparse else ""), r["perplexity"])
    print("  scored tokens %d in %d documents (%d skipped), log-likelihood %s" % (r["tokens"], r["documents"], r["skipped"], r["loglik"]))
    return r


def report_coherence(model, n):
    """mean UMass coherence of the labels' n best words and the five least coherent labels with those words"""
    idx, _ = model.top_words(n)
    coh = model.coherence(n, "umass")
    names = list(model.labelmap.keys())
    ok = np.flatnonzero(~np.isnan(coh))
    print("-----------------------------------")
    print("UMass coherence (top %d words), mean over %d of %d labels: " % (n, ok.shape[0], len(names)),
          np.mean(coh[ok]) if ok.shape[0] else float("nan"))
    for k in ok[np.argsort(coh[ok], kind="stable")[:5]]:
        print("  %-24s %10.3f  %s" % (names[k], coh[k], " ".join(model.v_to_w[int(v)] for v in idx[k] if v >= 0)))


def report_window_coherence(model, texts, n):
    """mean C_V coherence of the labels' n best words over the token lists ``texts`` and the five least coherent labels with those words"""
    idx, _ = model.top_words(n)
    coh = model.window_coherence(texts, n, "c_v")
    names = list(model.labelmap.keys())
    ok = np.flatnonzero(~np.isnan(coh))
    print("-----------------------------------")
    print("C_V coherence (top %d words), mean over %d of %d labels: " % (n, ok.shape[0], len(names)),
          np.mean(coh[ok]) if ok.shape[0] else float("nan"))
    for k in ok[np.argsort(coh[ok], kind="stable")[:5]]:
        print("  %-24s %10.3f  %s" % (names[k], coh[k], " ".join(model.v_to_w[int(v)] for v in idx[k] if v >= 0)))


def report_frex_words(model, n, weight):
    """every label's n FREX words (LabeledLDA.frex_words) next to its n most frequent ones"""
    frequent, _ = model.top_words(n)
    frex, _ = model.frex_words(n, weight)
    names = list(model.labelmap.keys())
    words = lambda row: " ".join(model.v_to_w[int(v)] for v in row if v >= 0)
    print("-----------------------------------")
    print("Label words (top %d): most frequent | FREX (weight %g):" % (n, weight))
    for k, name in enumerate(names):
        print("  %-24s %s | %s" % (name, words(frequent[k]), words(frex[k])))


def report_exclusivity(model, n, weight):
    """topic exclusivity of every label's n most probable words (LabeledLDA.exclusivity): the mean and the five lowest"""
    ex = model.exclusivity(n, weight)
    names = list(model.labelmap.keys())
    ok = np.flatnonzero(~np.isnan(ex))
    print("-----------------------------------")
    print("Exclusivity (FREX weight %g, top %d words), mean over %d labels: %.3f" % (weight, n, len(ok), np.mean(ex[ok]) if len(ok) else float("nan")))
    print("Least exclusive labels:")
    for k in ok[np.argsort(ex[ok], kind="stable")[:5]]:
        print("  %-24s %10.3f" % (names[k], ex[k]))


def report_label_words(model, n, lam, coherence_n=0, window_n=0, texts=None):
    """every label's n most distinctive words (LabeledLDA.label_words) next to its n most frequent ones; coherence_n / window_n > 0: the
    mean UMass / C_V coherence of both kinds of list"""
    frequent, _ = model.top_words(n)
    distinctive, _ = model.label_words(n, lam)
    names = list(model.labelmap.keys())
    words = lambda row: " ".join(model.v_to_w[int(v)] for v in row if v >= 0)
    print("-----------------------------------")
    print("Label words (top %d): most frequent | most distinctive (relevance %g):" % (n, lam))
    for k, name in enumerate(names):
        print("  %-24s %s | %s" % (name, words(frequent[k]), words(distinctive[k])))
    mean = lambda coh: np.mean(coh[~np.isnan(coh)]) if (~np.isnan(coh)).any() else float("nan")
    if coherence_n:
        print("UMass coherence (top %d words), mean: frequent %s, distinctive %s"
              % (coherence_n, mean(model.coherence(coherence_n, "umass")), mean(model.coherence(coherence_n, "umass", lam=lam))))
    if window_n:
        print("C_V coherence (top %d words), mean: frequent %s, distinctive %s"
              % (window_n, mean(model.window_coherence(texts, window_n, "c_v")), mean(model.window_coherence(texts, window_n, "c_v", lam=lam))))


def _header(lvl, it, corpus_file):
    print("Model:               Labeled LDA")
    print("Corpus:             ", "Abstracts" if corpus_file == "thesis_data3.csv" else "Full Texts")
    print("Label depth         ", lvl)
    print("# of Gibbs samples: ", int(it))
    print("-----------------------------------")


def report_device(model, test, th, lvl, it, corpus_file):
    """``report`` with the ranking and the per-document metrics on the device (ranking.rank_labels / ranking.metrics): the same
    lines; equal loads are ranked by label index where numpy's argsort in n_error leaves their order open."""
    from . import ranking
    _header(lvl, it, corpus_file)
    m = ranking.metrics(ranking.rank_labels(th, binary_yreal(test[1], model.labelmap), first=1, top_n=0))
    print("AUC ROC:                 ", m["auc"])
    print("one error:               ", m["one_error"])
    print("two error:               ", m["two_error"])
    print("F1 score (macro average) ", m["f1"])


def report(model, test, th, lvl, it, corpus_file):
    _header(lvl, it, corpus_file)
    y_bin = binary_yreal(test[1], model.labelmap)[:, 1:]        # the root label is in no label set
    th = th[:, 1:]
    keep = np.where(th.sum(axis=1) != 0)[0]                     # documents not assigned to 'root' entirely
    y_bin, th = y_bin[keep, :], th[keep, :]
    tps, tns, fps, fns, fprs, tprs = rates(th, y_bin)
    print("AUC ROC:                 ", macro_auc_roc(fprs, tprs))
    print("one error:               ", n_error(th, y_bin, 1))
    print("two error:               ", n_error(th, y_bin, 2))
    print("F1 score (macro average) ", get_f1(tps, fps, tns, fns))


def main(argv=None):
    opt, _ = build_parser().parse_args(argv)
    if opt.thinning == 0:
        opt.thinning = opt.it
    train, test = split_data(f=opt.file, d=opt.lvl)
    print("Starting training...")
    model = train_it(train, it=opt.it, s=opt.thinning, al=opt.alpha, be=opt.beta, l=opt.lower, u=opt.upper, em=opt.em_train,
                     em_sparse=opt.em_sparse)
    print("Testing test data, this may take a while...")
    th, _ = test_it(model, test, it=opt.it, thinning=opt.thinning)
    th = np.array(th)
    if opt.pickle:
        pickle.dump(model, open("LabeledLDA_model.pkl", "wb"))
        pickle.dump(test, open("LabeledLDA_testset.pkl", "wb"))
        pickle.dump(th, open("LabeledLDA_theta.pkl", "wb"))
    (report_device if opt.device_metrics else report)(model, test, th, opt.lvl, opt.it, opt.file)
    if opt.coherence:
        report_coherence(model, opt.coherence)
    if opt.window_coherence:
        report_window_coherence(model, train[0], opt.window_coherence)
    if opt.label_words:
        report_label_words(model, opt.label_words, opt.relevance, opt.coherence, opt.window_coherence, train[0])
    if opt.frex_words:
        report_frex_words(model, opt.frex_words, 0.5 if opt.frex_weight is None else opt.frex_weight)
    if opt.exclusivity:
        report_exclusivity(model, opt.exclusivity, 0.7 if opt.frex_weight is None else opt.frex_weight)
    if opt.heldout_perplexity:
        report_heldout(model, test, opt.it, opt.thinning)
    if opt.left_to_right:
        report_left_to_right(model, test, opt.left_to_right, sparse=opt.lr_sparse)
    if opt.shortlist:
        report_shortlist(model, test, opt.it, opt.thinning, opt.shortlist)
    if opt.heldout_em:
        report_heldout_em(model, test, opt.heldout_em, sparse=opt.em_sparse)
    if opt.em_foldin:
        report_em_foldin(model, test, opt.em_foldin)
    if opt.explain:
        report_explain(model, test, opt.explain, opt.em_foldin or 50)
    if opt.knn:
        report_knn(model, test, opt.it, opt.thinning, opt.knn)
    if opt.similar_labels:
        report_similar_labels(model, opt.similar_labels)
    if opt.label_report:
        report_labels(model, test, opt.it, opt.thinning)
    if opt.label_sets:
        report_label_sets(model, test, opt.it, opt.thinning)


if __name__ == "__main__":
    main()
